"""GPU: the drawing library (include/agt_draw.h) against its numpy statement (tests/overlay_numpy.py), byte for byte: no tolerance, no
case left out.  Frames are views into one flat buffer of random bytes with padded rows, padded frames and guard bytes on both sides,
and the WHOLE buffer is compared, so a byte written outside a frame's pixels shows.  The frames are small: 70 x 37 and 129 x 65 are no
multiple of the 32 x 8 tile in either direction and make 3 x 5 and 5 x 9 tiles."""
import itertools
import json
import logging

import numpy as np
import pytest

import overlay_numpy as on

pytestmark = pytest.mark.gpu
LOG = logging.getLogger("test"); LOG.setLevel(logging.CRITICAL)
SIZES = [(70, 37), (129, 65)]
TILE_W, TILE_H, CHUNK = 32, 8, 256
GUARD, ROW_PAD, FRAME_PAD = 96, 5, 13
RED, GREEN, BLUE, WHITE, ODD = (0, 0, 255), (0, 255, 0), (255, 0, 0), (255, 255, 255), (7, 130, 251)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


@pytest.fixture(scope="module")
def ov(torch_cuda):
    from accurate_aprilgroup_tracking_amd import drawlib, overlay
    assert drawlib.CHUNK == CHUNK
    return overlay


def check_raster(torch, ov, w, h, ch, lists, clear=False, seed=0, runs=1):
    """lists: one PRIM_DTYPE array [P] per frame (equal P).  Device against numpy over the whole padded buffer."""
    B, P = len(lists), len(lists[0])
    pitch = w * ch + ROW_PAD
    fs = pitch * h + FRAME_PAD
    flat = np.random.default_rng(seed).integers(0, 256, GUARD + B * fs + GUARD, dtype=np.uint8)
    host = flat.copy()
    for b in range(B):
        shape, strides = ((h, w), (pitch, 1)) if ch == 1 else ((h, w, 3), (pitch, 3, 1))
        on.raster(np.lib.stride_tricks.as_strided(host[GUARD + b * fs:], shape, strides), lists[b], clear)
    prims = ov.prims_tensor(np.stack(lists) if P else np.zeros((B, 0), on.PRIM_DTYPE), "cuda")
    outs = []
    for _ in range(runs):
        dev = torch.from_numpy(flat).cuda()
        frames = dev.as_strided((B, h, w) if ch == 1 else (B, h, w, 3), (fs, pitch, 1) if ch == 1 else (fs, pitch, 3, 1), GUARD)
        ov.draw_primitives(frames, prims, clear=clear)
        outs.append(dev.cpu().numpy())
    bad = np.flatnonzero(outs[0] != host)
    assert bad.size == 0, "%d bytes differ, the first at offset %d (frame bytes start at %d, frame stride %d, pitch %d)" % (bad.size, bad[0], GUARD, fs, pitch)
    assert all(np.array_equal(o, outs[0]) for o in outs[1:])
    return host


def geometry(w, h):
    """discs and segments on tile borders, frame edges and corners, clipped by every edge, through every tile, from outside to outside,
    of no length, of every size the issue names"""
    cx, cy = w // 2, h // 2
    g = [on.segment(-10, cy, w + 10, cy, 64, (40, 40, 40)),                       # covers the frame: crosses every tile
         on.disc(cx, cy, 64, (60, 20, 90)), on.disc(-40, -40, 64, ODD),
         on.disc(0, 0, 5, RED), on.disc(w - 1, 0, 5, GREEN), on.disc(0, h - 1, 5, BLUE), on.disc(w - 1, h - 1, 5, WHITE),
         on.disc(-3, cy, 5, RED), on.disc(w + 2, cy, 5, GREEN), on.disc(cx, -3, 5, BLUE), on.disc(cx, h + 2, 5, WHITE),
         on.disc(-6, 3, 5, ODD), on.disc(w + 5, 3, 5, ODD),                       # touch the frame with one column at most
         on.disc(TILE_W, TILE_H, 5, RED), on.disc(TILE_W - 1, TILE_H - 1, 5, GREEN), on.disc(2 * TILE_W, 3 * TILE_H, 0, WHITE),
         on.disc(TILE_W - 1, 2 * TILE_H, 0, BLUE), on.disc(0, 0, 0, ODD), on.disc(w - 1, h - 1, 0, ODD), on.disc(w, h, 0, ODD),
         on.segment(0, TILE_H - 1, w - 1, TILE_H - 1, 1, RED), on.segment(0, TILE_H, w - 1, TILE_H, 1, GREEN),
         on.segment(TILE_W - 1, 0, TILE_W - 1, h - 1, 1, BLUE), on.segment(TILE_W, 0, TILE_W, h - 1, 1, WHITE),
         on.segment(0, 0, w - 1, 0, 1, ODD), on.segment(0, h - 1, w - 1, h - 1, 2, RED), on.segment(0, 0, 0, h - 1, 2, GREEN),
         on.segment(w - 1, 0, w - 1, h - 1, 5, BLUE), on.segment(0, 0, w - 1, h - 1, 1, WHITE), on.segment(w - 1, 0, 0, h - 1, 2, ODD),
         on.segment(-20, -5, w + 20, h + 7, 5, RED), on.segment(w + 30, 10, -30, 20, 1, GREEN), on.segment(-50, -60, -20, h + 90, 64, BLUE),
         on.segment(cx, cy, cx, cy, 5, WHITE), on.segment(3, 3, 3, 3, 0, RED), on.segment(9, 3, 9, 3, 1, GREEN), on.segment(15, 12, 15, 12, 2, BLUE),
         on.segment(cx + 9, cy, cx + 9, cy, 64, ODD), on.segment(5, 20, 40, 27, 0, WHITE), on.segment(5, 30, 60, 30, 0, RED),
         on.segment(w - 1, h - 1, w - 1, h - 1, 5, GREEN), on.segment(0, 0, 0, 0, 5, BLUE)]
    return g


def scatter(w, h, count, seed):
    """`count` small primitives all over (and around) the frame, a few of them invalid"""
    r = np.random.default_rng(seed)
    out = []
    for i in range(count):
        c = tuple(int(v) for v in r.integers(1, 256, 3))
        x0, y0 = int(r.integers(-8, w + 8)), int(r.integers(-8, h + 8))
        k = i % 7
        if k in (0, 1, 2):
            out.append(on.disc(x0, y0, int(r.integers(0, 5)), c))
        elif k in (3, 4, 5):
            out.append(on.segment(x0, y0, x0 + int(r.integers(-12, 13)), y0 + int(r.integers(-12, 13)), int(r.integers(0, 4)), c))
        else:
            out.append(on.prim(int(r.integers(3, 9)), x0, y0, x0, y0, 3, c))
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_geometry_list_in_padded_frames(torch_cuda, ov, w, h, ch, B):
    g = geometry(w, h)
    lists = [on.prim_list(g[b:] + g[:b]) for b in range(B)]            # another painter's order in every frame
    check_raster(torch_cuda, ov, w, h, ch, lists, clear=False, seed=B)
    check_raster(torch_cuda, ov, w, h, ch, [l[3:] for l in lists], clear=True, seed=B + 10, runs=2)


@pytest.mark.parametrize("w,h", SIZES)
def test_every_geometry_primitive_alone(torch_cuda, ov, w, h):
    """P = 1, one frame per primitive: nothing painted later hides a wrong pixel"""
    g = geometry(w, h)
    check_raster(torch_cuda, ov, w, h, 3, [on.prim_list([p]) for p in g], clear=False)
    check_raster(torch_cuda, ov, w, h, 1, [on.prim_list([p]) for p in g], clear=True)


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("clear", [False, True])
def test_empty_list(torch_cuda, ov, ch, clear):
    host = check_raster(torch_cuda, ov, 70, 37, ch, [on.prim_list([])] * 2, clear=clear)
    pitch = 70 * ch + ROW_PAD
    first = np.lib.stride_tricks.as_strided(host[GUARD:], (37, 70 * ch), (pitch, 1))
    assert (not first.any()) if clear else first.any()


@pytest.mark.parametrize("P", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_lists_around_the_chunk_size(torch_cuda, ov, P):
    for (w, h), clear in zip(SIZES, (False, True)):
        lists = [on.prim_list(scatter(w, h, P, seed=P + b)) for b in range(2)]
        check_raster(torch_cuda, ov, w, h, 3, lists, clear=clear, runs=2)


def test_painters_order(torch_cuda, ov):
    """three overlapping primitives in all six orders, alone and astride the chunk boundary (list places 254 .. 257)"""
    w, h = 70, 37
    three = [on.disc(30, 8, 6, RED), on.segment(20, 4, 45, 14, 5, GREEN), on.disc(33, 10, 4, BLUE)]
    filler = scatter(w, h, CHUNK + 40, seed=5)
    alone, astride = [], []
    for order in itertools.permutations(range(3)):
        alone.append(on.prim_list([three[i] for i in order]))
        for start in (CHUNK - 2, CHUNK - 1):
            lst = list(filler)
            for k, i in enumerate(order):
                lst[start + k] = three[i]
            astride.append(on.prim_list(lst))
    hosts = check_raster(torch_cuda, ov, w, h, 3, alone, clear=True)
    assert len({hosts[GUARD + b * ((w * 3 + ROW_PAD) * h + FRAME_PAD):][:(w * 3 + ROW_PAD) * h].tobytes() for b in range(6)}) > 1
    check_raster(torch_cuda, ov, w, h, 3, astride, clear=False)
    check_raster(torch_cuda, ov, w, h, 1, astride, clear=True)


def test_invalid_primitives_paint_nothing(torch_cuda, ov):
    w, h = 70, 37
    a, b = on.disc(20, 20, 5, RED), on.segment(5, 5, 60, 30, 2, GREEN)
    bad = [on.prim(3, 20, 20, 20, 20, 5, WHITE), on.prim(-1, 20, 20, 20, 20, 5, WHITE), on.prim(1 << 30, 20, 20, 20, 20, 5, WHITE)]
    for v in (32768, -32768, 1 << 30, -(1 << 30)):
        bad += [on.disc(v, 20, 5, WHITE), on.prim(on.DISC, 20, v, 20, 20, 5, WHITE), on.segment(20, 20, v, 20, 5, WHITE),
                on.segment(20, 20, 20, v, 5, WHITE), on.prim(on.DISC, 20, 20, v, 20, 5, WHITE)]
    bad += [on.disc(20, 20, -1, WHITE), on.disc(20, 20, 65, WHITE), on.segment(0, 0, 60, 30, -1, WHITE), on.segment(0, 0, 60, 30, 65, WHITE),
            on.disc(20, 20, -(1 << 31), WHITE), on.disc(20, 20, (1 << 31) - 1, WHITE)]
    lst = [a]
    for p in bad:
        lst += [p, b if len(lst) % 4 == 1 else a]
    second = bad + [a, b] + [on.prim(on.NONE, 20, 20, 40, 30, 5, WHITE)] * (len(lst) - len(bad) - 2)       # (equal P in both frames)
    host = check_raster(torch_cuda, ov, w, h, 3, [on.prim_list(lst), on.prim_list(second)], clear=True)
    only = on.raster(np.zeros((h, w, 3), np.uint8), on.prim_list([a, b]))
    got = np.lib.stride_tricks.as_strided(host[GUARD + (w * 3 + ROW_PAD) * h + FRAME_PAD:], (h, w, 3), (w * 3 + ROW_PAD, 3, 1))
    assert np.array_equal(got, only)
    # the limits themselves are valid
    edge = [on.segment(-32767, 20, 32767, 20, 1, RED), on.segment(20, -32767, 20, 32767, 64, GREEN), on.disc(20, 20, 64, BLUE), on.disc(-32767, 32767, 64, ODD)]
    check_raster(torch_cuda, ov, w, h, 3, [on.prim_list(edge)], clear=False)


@pytest.mark.parametrize("T", [1, 64])
def test_longest_segment_does_not_overflow(torch_cuda, ov, T):
    """(-32767, -32767) -> (32767, 32766) through a 129 x 65 frame: the squared cross product passes 2^64"""
    lst = on.prim_list([on.segment(-32767, -32767, 32767, 32766, T, WHITE), on.segment(32767, -32766, -32767, 32767, T, RED),
                        on.segment(-32767, 30, 32767, 31, T, GREEN)])
    host = check_raster(torch_cuda, ov, 129, 65, 3, [lst, lst[::-1].copy()], clear=True)
    assert host[GUARD:GUARD + (129 * 3 + ROW_PAD) * 65].any()


def special_points(w, h, dtype):
    """entry 0: the values the issue names; entries 1, 2: points about the frame"""
    inf, nan = np.inf, np.nan
    e0 = [[0.5, 1.5], [2.5, 3.5], [-0.4, -0.4], [w - 0.5, 4.0],             # half to even; -0.4; width - 0.5; whole tag inside for int()
          [10.0, 10.0], [20.0, nan], [20.0, 20.0], [10.0, 20.0],
          [inf, 5.0], [5.0, -inf], [1e30, 5.0], [5.0, -1e30],
          [w - 0.51, h - 0.51], [w - 1.0, h - 1.0], [0.0, 0.0], [-0.5, -0.5],    # -0.5 rounds to -0: inside
          [4.5, h - 0.5], [w, 3.0], [3.0, h], [-1.0, 3.0],
          [30.25, 12.75], [44.5, 12.5], [43.5, 25.5], [31.5, 26.49]]
    r = np.random.default_rng(3)
    rest = r.uniform(-6, max(w, h) + 6, (2, len(e0), 2))
    return np.concatenate([np.array(e0)[None], rest]).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("w,h", SIZES)
def test_pose_lists_records(torch_cuda, ov, w, h, dtype):
    torch = torch_cuda
    pts = special_points(w, h, dtype)
    B, n = pts.shape[:2]
    dev_pts = torch.from_numpy(pts).cuda()
    for gate in (None, np.array([1.0, 0.0, np.nan]), np.array([1.0, 1.0 + 2.0 ** -52, -1.0]), np.array([0.0, 1.0, 1.0])):
        ok = None
        if gate is not None:
            state = torch.full((B, 7), 1.0, dtype=torch.float64, device="cuda")         # a record block: the gate is a column of it
            state[:, 2] = torch.from_numpy(gate).cuda()
            ok = state[:, 2]
        want = on.pose_lists(pts, w, h, gate, radius=5, thickness=3, dot_color=RED, line_color=ODD)
        for _ in range(2):
            dots, outline = ov.pose_lists(dev_pts, (w, h), ok, radius=5, thickness=3, dot_color=RED, line_color=ODD)
            assert dots.cpu().numpy().tobytes() == want[0].tobytes() and outline.cpu().numpy().tobytes() == want[1].tobytes()
    d = ov.prims_numpy(ov.pose_lists(dev_pts, (w, h))[0])[0]
    assert (d["x0"][0], d["y0"][0], d["x0"][1], d["y0"][1]) == (0, 2, 2, 4) and d["kind"][2] == on.DISC and d["kind"][3] == (on.DISC if w % 2 else on.NONE)


def test_draw_pose_door(torch_cuda, ov):
    torch = torch_cuda
    w, h = 129, 65
    pts = special_points(w, h, np.float64)
    B = pts.shape[0]
    base = np.random.default_rng(1).integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    gate = np.array([1.0, 0.0, 1.0])
    frames, draw = torch.from_numpy(base).cuda(), torch.full((B, h, w, 3), 9, dtype=torch.uint8, device="cuda")
    ov.draw_pose(frames, draw, torch.from_numpy(pts).cuda(), ok=torch.from_numpy(gate).cuda())
    for b in range(B):
        f, d = on.draw_pose(base[b].copy(), np.full((h, w, 3), 9, np.uint8), pts[b], drawn=gate[b] == 1.0)
        assert np.array_equal(frames[b].cpu().numpy(), f) and np.array_equal(draw[b].cpu().numpy(), d)
    assert np.array_equal(frames[1].cpu().numpy(), base[1]) and not draw[1].any() and draw[0].any()
    # gray frames take colour[0]: the dots are 0, the outline 255
    g, gd = torch.from_numpy(base[..., 0].copy()).cuda(), torch.empty((B, h, w), dtype=torch.uint8, device="cuda")
    ov.draw_pose(g, gd, torch.from_numpy(pts.astype(np.float32)).cuda())
    for b in range(B):
        f, d = on.draw_pose(base[b, :, :, 0].copy(), np.zeros((h, w), np.uint8), pts[b].astype(np.float32))
        assert np.array_equal(g[b].cpu().numpy(), f) and np.array_equal(gd[b].cpu().numpy(), d)


def test_cv_hip_circle_and_line_in_place(torch_cuda):
    from accurate_aprilgroup_tracking_amd import cv_hip
    base = np.random.default_rng(2).integers(0, 256, (65, 129, 3), dtype=np.uint8)
    img, want = base.copy(), base.copy()
    assert cv_hip.circle(img, (20, 30), 5, (0, 0, 255), -1) is img
    cv_hip.line(img, (3, 60), (120, 2), (255, 255, 255), 5, cv_hip.LINE_AA)
    cv_hip.line(img, (np.int64(-9), 10), (140, np.int32(12)), (1, 2, 3))
    on.raster(want, on.prim_list([on.disc(20, 30, 5, RED), on.segment(3, 60, 120, 2, 5, WHITE), on.segment(-9, 10, 140, 12, 1, (1, 2, 3))]))
    assert np.array_equal(img, want)
    # a view (the ROI crop of the live loop) and a gray image
    view, wview = img[5:40, 7:90], want[5:40, 7:90]
    cv_hip.circle(view, (0, 0), 5, (9, 8, 7), thickness=cv_hip.FILLED)
    on.raster(wview, on.prim_list([on.disc(0, 0, 5, (9, 8, 7))]))
    assert np.array_equal(img, want)
    gray, wgray = base[:, :, 1].copy(), base[:, :, 1].copy()
    cv_hip.line(gray, (0, 0), (128, 64), 200, 2)
    cv_hip.circle(gray, (64, 32), 5, (0, 0, 255), -1)
    on.raster(wgray, on.prim_list([on.segment(0, 0, 128, 64, 2, (200, 200, 200)), on.disc(64, 32, 5, RED)]))
    assert np.array_equal(gray, wgray)
    for call in (lambda: cv_hip.circle(img, (5, 5), 5, RED, 1), lambda: cv_hip.circle(img, (5, 5), 65, RED, -1), lambda: cv_hip.line(img, (0, 0), (5, 5), RED, 0),
                 lambda: cv_hip.line(img, (0, 0), (40000, 5), RED, 1), lambda: cv_hip.line(img.astype(np.float32), (0, 0), (5, 5), RED, 1)):
        with pytest.raises(cv_hip.error):
            call()
    assert np.array_equal(img, want)


def test_stream_tracker_draw_overlay(torch_cuda, ov, seq640):
    """two streams over the synthetic clip; stream 1 is handed a blank frame at the last step and fails the gate: its frame stays
    untouched, its drawing frame is black; the others equal numpy applied to the projected points of the read-back records"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import cv_hip, hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    w, h = s.width, s.height
    frames = torch.from_numpy(s.frames()).cuda()
    trk = StreamTracker(w, h, s.obj, s.K, s.dist, n_streams=2)
    c0 = torch.from_numpy(np.stack([s.corners(0), s.corners(0)])).cuda().contiguous()
    trk.reset(torch.stack([frames[0], frames[0]]).contiguous(), c0)
    so = trk.new_state_buffer()
    draw = torch.full((2, h, w, 3), 77, dtype=torch.uint8, device="cuda")
    for k in (1, 2):
        f = torch.stack([frames[k], frames[k] if k == 1 else torch.zeros_like(frames[k])]).contiguous()
        trk.step(f, so)
        trk.join()
        bgr = torch.stack([f, f // 2, 255 - f], dim=3).contiguous()
        before = bgr.cpu().numpy()
        points = trk.draw_overlay(bgr, draw, so)
        st, pts = so.cpu().numpy(), points.cpu().numpy()
        assert st[0, H.ST_OK] == 1.0 and st[1, H.ST_OK] == (1.0 if k == 1 else 0.0), "frame %d: %s" % (k, st[:, H.ST_OK])
        for b in range(2):
            accepted = st[b, H.ST_OK] == 1.0
            f_want, d_want = on.draw_pose(before[b].copy(), np.full((h, w, 3), 77, np.uint8), pts[b], drawn=accepted)
            assert np.array_equal(bgr[b].cpu().numpy(), f_want) and np.array_equal(draw[b].cpu().numpy(), d_want), (k, b)
            if accepted:
                ref, _ = cv_hip.projectPoints(s.obj.astype(np.float32), st[b, :3], st[b, 3:6], s.K, s.dist)
                assert np.abs(ref.reshape(-1, 2) - pts[b]).max() < 1e-3
                assert (bgr[b].cpu().numpy() != before[b]).any() and draw[b].any()
            else:
                assert np.array_equal(bgr[b].cpu().numpy(), before[b]) and not draw[b].any()


class FirstFrameDetector:
    """every tag in the first frame, nothing afterwards: the LK path carries the stream"""

    def __init__(self, sc):
        from accurate_aprilgroup_tracking_amd import formats
        self.sc, self.k, self.F = sc, 0, formats
        self.tag_ids = [int(t) for t in sc.group["tags"].keys()]

    def __call__(self, gray):
        k = self.k
        self.k += 1
        if k:
            return []
        c = self.sc.corners(0).reshape(-1, 4, 2)
        return [self.F.make_detection(t, c[i], decision_margin=75.0) for i, t in enumerate(self.tag_ids)]


MODES = ["detector_present", "one_call_path", "raw_frames_with_distortion", "gray_frames", "gray_raw_frames_with_distortion"]


@pytest.mark.parametrize("mode", MODES)
def test_pose_detector_draws_the_same_on_both_backends(torch_cuda, tmp_path, seq640, seq640_dist, mode):
    """PoseDetector(backend="stream", draw=True) against PoseDetector(backend="cv", cv=cv_hip, draw=True) on the same frames, BGR and
    gray: the same bytes in overlay and drawing frame, both (H, W, 3); and drawing changes no pose -- the cv backend with draw=True
    gives bit for bit the poses it gives without (on a gray frame the dots must not land in the array LK tracks from)"""
    from accurate_aprilgroup_tracking_amd import cv_hip
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    dist, gray = mode.endswith("with_distortion"), mode.startswith("gray")
    sc = seq640_dist if dist else seq640
    (tmp_path / "april_group.json").write_text(json.dumps(sc.group))

    class Det(PoseDetector):
        DIRPATH = str(tmp_path)
    host = Det(LOG, sc.K, sc.dist, True, cv=cv_hip, detector=FirstFrameDetector(sc), draw=True)
    plain = Det(LOG, sc.K, sc.dist, True, cv=cv_hip, detector=FirstFrameDetector(sc))
    dev = Det(LOG, sc.K, sc.dist, True, detector=FirstFrameDetector(sc), backend="stream", draw=True)
    off = Det(LOG, sc.K, sc.dist, True, detector=FirstFrameDetector(sc), backend="stream")
    assert host.draw_frame is None and dev.draw_frame is None and dev.overlay is None
    drawn = 0
    for k in range(3):
        g = sc.frame(k)
        frame = g.copy() if gray else np.ascontiguousarray(np.stack([g, g, g], axis=2))
        for d in (host, plain, dev, off):
            if dist:
                d.step(frame.copy())
            else:
                d._detect_and_get_pose(frame.copy())
            if mode != "detector_present" and k == 0:
                d.detector = None
        assert off.draw_frame is None and off.overlay is None and plain.draw_frame is None and plain.overlay is None
        assert (host.last_error is None) == (dev.last_error is None) == (plain.last_error is None)
        if plain.last_error is not None:
            assert host.last_error == plain.last_error, "frame %d: drawing changed the error" % k
            assert all(np.array_equal(a, b) for a, b in zip(host.last_pose, plain.last_pose)), "frame %d: drawing changed the pose" % k
        assert dev.overlay.is_cuda and dev.draw_frame.is_cuda and tuple(dev.overlay.shape) == host.img.shape == tuple(dev.draw_frame.shape)
        assert host.overlay is host.img and host.img.ndim == 3 and host.img.shape[2] == 3 and host.draw_frame.shape == host.img.shape
        assert np.array_equal(dev.overlay.cpu().numpy(), host.img), "frame %d: overlay" % k
        assert np.array_equal(dev.draw_frame.cpu().numpy(), host.draw_frame), "frame %d: drawing frame" % k
        drawn += int(host.draw_frame.any())
        if not dist:
            assert host.last_error is not None and host.last_error < 2 and host.draw_frame.any(), "frame %d is not drawn" % k
            colour = frame if not gray else np.repeat(frame[:, :, None], 3, axis=2)
            assert (host.img != colour).any() and np.array_equal(dev.img, frame)
            red = (host.img != colour).any(axis=2)
            assert np.array_equal(host.img[red], np.broadcast_to(np.uint8([0, 0, 255]), (int(red.sum()), 3)))
    print("%s: %d of 3 frames drawn" % (mode, drawn))
    assert drawn >= 1, "no frame passed the gate: the undistort-and-ROI draw path was not exercised"
