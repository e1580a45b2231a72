"""-m gpu: the chessboard corner finder (include/agt_chess.h) against the numpy statement of its rule (tests/chessboard_numpy.py) --
the response and the candidates byte for byte (the rule is integer), the refined points within 1e-8 px with equal verdicts and two runs
bitwise equal -- at the smallest shapes at which the kernels can go wrong; then end to end on the rendered boards of
tests/chess_scenes.py, through chessboard.find_chessboard, cv_hip.findChessboardCorners and into calibrate_camera."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import chess_scenes as S            # noqa: E402
import chessboard_numpy as cb       # noqa: E402
from test_chessboard import MEASURED, bound          # noqa: E402

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 16             # ch_response's staging tile
REFINE_TOL = 1e-8                   # px: FP64 sums of at most 23 x 23 terms below 2^20 through 2 x 2 systems conditioned under 1e6


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    torch.cuda.set_device(0)
    return torch


def texture(h, w, seed, smooth=True):
    """a random frame; smoothed so that its response has well separated maxima of many heights"""
    from scipy import ndimage
    a = np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.float64)
    if smooth:
        a = ndimage.uniform_filter(a, 3, mode="nearest")
        a = (a - a.min()) * (255.0 / (a.max() - a.min()))
    return np.rint(a).astype(np.uint8)


def device_corners(torch, frames, max_candidates=1024, finder=None, **options):
    """host frames [B, H, W] (or a cuda tensor) -> (tables i32 [B, C, 3], counts i32 [B, 4], records [B, C] structured) on the host"""
    from accurate_aprilgroup_tracking_amd import chessboard
    f = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.array(frames)).cuda()
    if finder is None:
        finder = chessboard.ChessboardFinder(f.shape[2], f.shape[1], f.shape[0], max_candidates)
    out = finder.corners(f, **options)
    torch.cuda.synchronize()
    return out.candidates.cpu().numpy(), out.counts.cpu().numpy(), chessboard.records_numpy(out.records)


def statement_corners(frames, max_candidates=1024, **options):
    parts = [cb.corners(f, max_candidates, **options) for f in frames]
    return tuple(np.stack([p[k] for p in parts]) for k in range(3))


def same_candidates(got, want, what=""):
    assert got[1].tolist() == want[1].tolist(), (what, "counts", got[1].tolist(), want[1].tolist())
    assert got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes(), (what, "candidates differ")


def same_records(got, want, what=""):
    """verdict bytes equal, reserved bytes zero, points within REFINE_TOL and their f32 the rounding of the f64"""
    assert got.shape == want.shape and np.array_equal(got["verdict"], want["verdict"]), (what, got["verdict"].tolist(), want["verdict"].tolist())
    assert not got["reserved"].any()
    d = max(np.abs(got["x"] - want["x"]).max(), np.abs(got["y"] - want["y"]).max()) if got.size else 0.0
    assert d <= REFINE_TOL, (what, d)
    assert np.array_equal(got["xf"], got["x"].astype(np.float32)) and np.array_equal(got["yf"], got["y"].astype(np.float32))
    assert np.allclose(got["det"], want["det"], rtol=1e-9, atol=0) and np.allclose(got["shift"], want["shift"], rtol=0, atol=REFINE_TOL)
    return d


# ---- stage 1: the response, byte for byte

RESPONSE_SHAPES = [(11, 11), (12, 11), (11, 12), (TILE_W - 1, TILE_H - 1), (TILE_W, TILE_H), (TILE_W + 1, TILE_H + 1), (2 * TILE_W + 1, 2 * TILE_H + 1)]


@pytest.mark.parametrize("w,h", RESPONSE_SHAPES)
def test_response_equals_the_statement(torch_cuda, w, h):
    """random frames (rough and smoothed) and frames of one constant value, as one batch per size"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import chessboard
    frames = np.stack([texture(h, w, 1, smooth=False), texture(h, w, 2), np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8), np.full((h, w), 93, np.uint8)])
    got = chessboard.ChessboardFinder(w, h, len(frames)).response(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and tuple(got.shape) == frames.shape
    got = got.cpu().numpy()
    want = np.stack([cb.response(f) for f in frames])
    assert got.tobytes() == want.tobytes(), "%d responses differ" % int((got != want).sum())
    assert want[0].any() and not want[2:].any(), "a constant frame has no response anywhere"
    if (w, h) == (11, 11):
        assert np.count_nonzero(want[0]) == 1 and want[0][5, 5] != 0, "exactly one pixel with a ring"


def test_response_pitch_stride_and_batch(torch_cuda):
    """B = 3 in a buffer whose rows are 13 bytes longer than the frame and whose frame stride is larger than a frame, the frames lying
    inside a bright border that must not leak in; a handle made for larger frames"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import chessboard
    w, h = TILE_W + 7, TILE_H + 5
    frames = np.stack([texture(h, w, k) for k in (3, 4, 5)])
    buf = torch.full((3, h + 9, w + 13), 255, dtype=torch.uint8, device="cuda")
    view = buf[:, 4:4 + h, 5:5 + w]
    view.copy_(torch.from_numpy(frames).cuda())
    assert view.stride(1) == w + 13 and view.stride(0) == (h + 9) * (w + 13) and not view.is_contiguous()
    fd = chessboard.ChessboardFinder(200, 100, 3)
    got = fd.response(view)
    torch.cuda.synchronize()
    assert got.cpu().numpy().tobytes() == np.stack([cb.response(f) for f in frames]).tobytes()
    same_candidates(device_corners(torch, view, finder=fd, min_response=1)[:2], statement_corners(frames, min_response=1)[:2], "view")
    one = fd.response(view[1:2])
    torch.cuda.synchronize()
    assert one.cpu().numpy()[0].tobytes() == cb.response(frames[1]).tobytes()


# ---- stage 2: the candidates, in value and in order

def test_ties_inside_one_window_go_to_the_smallest_index(torch_cuda):
    """a frame mirrored left to right and top to bottom: the response is mirrored too, so next to the axes equal responses fall into
    one suppression window"""
    q = texture(14, 16, 7)
    top = np.concatenate([q, q[:, -2::-1]], axis=1)
    frame = np.concatenate([top, top[-2::-1]], axis=0)
    R = cb.response(frame)
    assert np.array_equal(R, R[:, ::-1]) and np.array_equal(R, R[::-1])
    for nms in (1, 2, 3, 5):
        kw = dict(min_response=1, rel_pct=0, nms=nms)
        want = statement_corners(frame[None], 256, **kw)
        same_candidates(device_corners(torch_cuda, frame[None], 256, **kw)[:2], want[:2], "nms %d" % nms)
        n = want[1][0, 1]
        assert n > 0 and np.all(np.diff(want[0][0, :n, 1] * frame.shape[1] + want[0][0, :n, 0]) > 0), "raster order"
    # the tie rule decided somewhere: a kept candidate whose mirror image has the same response inside its window and was dropped
    t = statement_corners(frame[None], 256, min_response=1, rel_pct=0, nms=3)[0][0]
    kept = {(int(x), int(y)) for x, y, r in t if r > 0}
    W, H = frame.shape[1], frame.shape[0]
    assert any(((W - 1 - x, y) not in kept and 0 < abs(W - 1 - 2 * x) <= 3) or ((x, H - 1 - y) not in kept and 0 < abs(H - 1 - 2 * y) <= 3) for x, y in kept)


def test_overflow_keeps_the_first_and_writes_nothing_behind_the_table(torch_cuda):
    """a fine checker has an X-corner every 6 pixels: far more than max_candidates = 8"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import chessboard
    y, x = np.mgrid[0:48, 0:64]
    frame = np.where(((x // 6) + (y // 6)) % 2 == 0, 20, 230).astype(np.uint8)
    full = statement_corners(frame[None], 1024)
    assert full[1][0, 0] > 30 and full[1][0, 3] == 0
    C = 8
    want = statement_corners(frame[None], C)
    assert want[1][0].tolist() == [full[1][0, 0], C, full[1][0, 2], cb.FLAG_CANDIDATES] and want[0][0].tobytes() == full[0][0, :C].tobytes()
    fd = chessboard.ChessboardFinder(64, 48, 1, C)
    sizes = [C * 12, 16, C * 48]
    bufs = [torch.full((n + 128,), 0xA5, dtype=torch.uint8, device="cuda") for n in sizes]
    f = torch.from_numpy(frame[None]).cuda()
    from accurate_aprilgroup_tracking_amd.cv_hip import _raw_stream
    fd._finder(0).corners(_raw_stream(0), f.data_ptr(), 64, 64 * 48, 64, 48, 1, None, *[b[64:].data_ptr() for b in bufs])
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for b, n in zip(host, sizes):
        assert np.all(b[:64] == 0xA5) and np.all(b[64 + n:] == 0xA5), "the words in front of and behind the table are untouched"
    got = (host[0][64:64 + sizes[0]].view(np.int32).reshape(1, C, 3), host[1][64:64 + 16].view(np.int32).reshape(1, 4),
           host[2][64:64 + sizes[2]].view(cb.RECORD_DTYPE).reshape(1, C))
    same_candidates(got[:2], want[:2], "overflow")
    same_records(got[2], want[2], "overflow")


@pytest.mark.parametrize("nms", range(1, 9))
def test_every_suppression_radius(torch_cuda, nms):
    frame = texture(2 * TILE_H + 9, TILE_W + 9, 11)
    kw = dict(min_response=1, rel_pct=0, nms=nms)
    want = statement_corners(frame[None], 2048, **kw)
    same_candidates(device_corners(torch_cuda, frame[None], 2048, **kw)[:2], want[:2])
    assert want[1][0, 1] > 0 and want[1][0, 3] == 0


def test_maxima_next_to_the_border_and_the_thresholds(torch_cuda):
    """a rough frame at nms = 1 has maxima in the first and last rows and columns that have a ring; min_response and rel_pct at the
    value of a candidate and one above it"""
    frame = texture(40, 47, 14, smooth=False)
    kw = dict(min_response=1, rel_pct=0, nms=1)
    want = statement_corners(frame[None], 2048, **kw)
    t = want[0][0, :want[1][0, 1]]
    assert {5, 47 - 6} <= set(t[:, 0].tolist()) and {5, 40 - 6} <= set(t[:, 1].tolist())
    same_candidates(device_corners(torch_cuda, frame[None], 2048, **kw)[:2], want[:2], "border")
    r, rmax = int(np.sort(t[:, 2])[len(t) // 2]), int(want[1][0, 2])
    pct = (100 * r) // rmax
    for kw in (dict(min_response=r), dict(min_response=r + 1), dict(min_response=1, rel_pct=pct), dict(min_response=1, rel_pct=pct + 1), dict(min_response=1, rel_pct=100),
               dict(min_response=2 ** 31 - 1)):
        kw = dict(dict(nms=1, rel_pct=0), **kw)
        want = statement_corners(frame[None], 2048, **kw)
        same_candidates(device_corners(torch_cuda, frame[None], 2048, **kw)[:2], want[:2], str(kw))
    assert want[1][0].tolist() == [0, 0, rmax, 0]


# ---- stage 3: the saddle points

@pytest.mark.parametrize("kw", [dict(), dict(half=3), dict(half=11, iters=4), dict(half=1, iters=64, max_shift=64.0), dict(iters=1), dict(max_shift=0.05),
                                dict(min_det=5e9)], ids=str)
def test_refined_points_equal_the_statement(torch_cuda, kw):
    """clean and noisy view of the 640 x 480 scenes, and a rough texture whose maxima are no saddle points (verdicts of every kind)"""
    frames = np.stack([S.view("cam5", 0)[0], S.view("cam5", 1, True)[0], np.pad(texture(100, 200, 17), ((0, 380), (0, 440)), constant_values=128)])
    want = statement_corners(frames, 256, **kw)
    got = device_corners(torch_cuda, frames, 256, **kw)
    same_candidates(got[:2], want[:2], str(kw))
    d = same_records(got[2], want[2], str(kw))
    v = want[2]["verdict"][0, :want[1][0, 1]]
    good = want[2][0, :want[1][0, 1]][v == cb.OK]
    print("%s: largest difference %.3g px; verdicts of the batch %s; smallest det of a good corner %.3g" %
          (kw, d, np.bincount(np.concatenate([want[2]["verdict"][b, :want[1][b, 1]] for b in range(3)]), minlength=4).tolist(),
           good["det"].min() if len(good) else np.nan))
    again = device_corners(torch_cuda, frames, 256, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), "two runs are bitwise equal"


def test_window_at_the_borders_and_the_canary_margin(torch_cuda):
    """seeds whose window just fits and just does not at each border, and seeds far outside, on a frame that lies inside a larger
    buffer: the results equal the statement's on the frame alone whatever the margin holds, and the margin is not written"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import chessboard
    w, h, half = 61, 47, 5
    frame = texture(h, w, 19)
    xs = [half, half + 1, w - half - 3, w - half - 2]
    ys = [half, half + 1, h - half - 3, h - half - 2]
    seeds = [(x, 23) for x in xs] + [(30, y) for y in ys] + [(x, y) for x in xs[:2] for y in ys[2:]] + [(-1, 23), (30, -7), (w, 23), (30, h + 100), (2 ** 31 - 1, 5), (-2 ** 31, 5)]
    C = len(seeds) + 3
    table = np.zeros((1, C, 3), np.int32)
    table[0, :len(seeds), :2] = seeds
    table[0, len(seeds):] = 30                      # behind the count: never read as seeds
    counts = np.array([[len(seeds), len(seeds), 0, 0]], np.int32)
    # one iteration: the verdict is BORDER exactly when the window does not fit at the seed (on a texture the estimate wanders, and
    # more iterations may carry a window that fitted out of the frame: the last round below)
    kw = dict(half=half, min_det=0.0, max_shift=2.0, iters=1)
    want = cb.refine(frame, table[0], counts[0], **kw)
    fit = [x >= half + 1 and x <= w - half - 3 and y >= half + 1 and y <= h - half - 3 for x, y in seeds]
    assert [v != cb.BORDER for v in want["verdict"][:len(seeds)]] == fit and sum(fit) == 5 and not want[len(seeds):].tobytes().strip(b"\0")
    fd = chessboard.ChessboardFinder(w, h, 1, C)
    results = []
    for canary in (0, 255, 0x5A, -1):
        if canary < 0:
            canary, kw = 0x33, dict(kw, iters=10)
            want = cb.refine(frame, table[0], counts[0], **kw)
            results = []
        buf = torch.full((1, h + 16, w + 24), canary, dtype=torch.uint8, device="cuda")
        view = buf[:, 8:8 + h, 12:12 + w]
        view.copy_(torch.from_numpy(frame[None]).cuda())
        rec = fd.refine(view, torch.from_numpy(table).cuda(), torch.from_numpy(counts).cuda(), **kw)
        torch.cuda.synchronize()
        results.append(chessboard.records_numpy(rec)[0])
        b = buf.cpu().numpy()[0]
        b[8:8 + h, 12:12 + w] = canary
        assert np.all(b == canary) and np.array_equal(view.cpu().numpy()[0], frame), "nothing is written"
        if len(results) == 3:
            assert results[0].tobytes() == results[1].tobytes() == results[2].tobytes(), "no byte of the margin is read"
        same_records(results[-1], want, "borders, margin %d" % canary)
    # a count larger than the table or negative is clamped
    for n, filled in ((10 ** 6, C), (-5, 0)):
        rec = fd.refine(torch.from_numpy(frame[None]).cuda(), torch.from_numpy(table).cuda(), torch.tensor([[0, n, 0, 0]], dtype=torch.int32, device="cuda"), **kw)
        torch.cuda.synchronize()
        same_records(chessboard.records_numpy(rec)[0], cb.refine(frame, table[0], [0, filled, 0, 0], **kw), "count %d" % n)


def test_argument_errors_by_value(torch_cuda):
    """on a live handle: sizes under 11 or over the handle's, B over max_batch, pitch, stride, NULL pointers, every option's range"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import chessboard, chesslib as Q
    fd = chessboard.ChessboardFinder(64, 48, max_batch=2, max_candidates=16)
    ok = torch.from_numpy(texture(48, 64, 23)[None]).cuda()
    for frames in (torch.zeros((1, 10, 64), dtype=torch.uint8, device="cuda"), torch.zeros((1, 48, 10), dtype=torch.uint8, device="cuda"),
                   torch.zeros((3, 48, 64), dtype=torch.uint8, device="cuda"), torch.zeros((1, 49, 64), dtype=torch.uint8, device="cuda")):
        for call in (fd.corners, fd.response, fd.candidates):
            with pytest.raises(Q.ChessError, match="AGT_CHESS_ERR_ARG"):
                call(frames)
    for kw in (dict(min_response=0), dict(rel_pct=-1), dict(rel_pct=101), dict(nms=0), dict(nms=Q.MAX_NMS + 1), dict(half=0), dict(half=Q.MAX_HALF + 1), dict(iters=0),
               dict(iters=Q.MAX_ITERS + 1), dict(max_shift=0.0), dict(max_shift=64.5), dict(max_shift=float("inf")), dict(min_det=-1.0), dict(min_det=float("inf"))):
        for call in (fd.corners, fd.candidates):
            with pytest.raises(Q.ChessError, match="AGT_CHESS_ERR_ARG"):
                call(ok, **kw)
    h = fd._finder(0)
    good = dict(frames=ok.data_ptr(), pitch=64, stride=64 * 48, w=64, h=48, B=1, cands=64, counts=64, records=64)

    def call(**kw):
        a = dict(good, **kw)
        return h.L.agt_chess_corners(h.h, None, a["frames"], a["pitch"], a["stride"], a["w"], a["h"], a["B"], None, a["cands"], a["counts"], a["records"])
    for kw in (dict(w=10), dict(h=10), dict(w=65), dict(h=49), dict(B=0), dict(B=3), dict(pitch=63), dict(B=2, stride=64 * 47 + 63), dict(frames=None), dict(cands=None),
               dict(counts=None), dict(records=None)):
        assert call(**kw) == Q.ERR_ARG, kw
    assert h.L.agt_chess_response(h.h, None, ok.data_ptr(), 64, 64 * 48, 64, 48, 1, None) == Q.ERR_ARG
    assert h.L.agt_chess_refine(h.h, None, ok.data_ptr(), 64, 64 * 48, 64, 48, 1, None, None, 64, 64) == Q.ERR_ARG
    bad = Q.options(); bad.reserved0 = 1
    assert h.L.agt_chess_candidates(h.h, None, ok.data_ptr(), 64, 64 * 48, 64, 48, 1, bad, 64, 64) == Q.ERR_ARG
    # and the handle still works
    same_candidates(device_corners(torch, ok, 16, finder=fd, min_response=1)[:2], statement_corners(ok.cpu().numpy(), 16, min_response=1)[:2], "after the refusals")


# ---- end to end

@pytest.mark.parametrize("name,noisy", sorted(MEASURED))
def test_every_view_is_found_and_ordered_as_the_truth(torch_cuda, name, noisy):
    """within the bound the CPU test sets for the statement, plus 1e-6"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import chessboard
    views = S.class_views(name, noisy)
    frames = torch.from_numpy(np.stack([f for f, _ in views])).cuda()
    found = chessboard.find_chessboard(frames, S.PATTERN)
    errs = []
    for k, ((ok, pts), (_, truth)) in enumerate(zip(found, views)):
        assert ok and pts.dtype == np.float32 and pts.shape == (54, 2), (name, k)
        e = np.hypot(*(pts.astype(np.float64) - truth).T)
        assert e.max() < 1.0, "view %d is ordered as the truth" % k
        errs.append(e)
    e = np.concatenate(errs)
    rms, worst = float(np.sqrt((e ** 2).mean())), float(e.max())
    print("%s noisy=%s: device RMS %.4f px, worst %.4f px (bounds %.4f, %.4f)" % ((name, noisy, rms, worst) + bound(name, noisy)))
    assert rms <= bound(name, noisy)[0] + 1e-6 and worst <= bound(name, noisy)[1] + 1e-6


def test_no_board_and_half_a_board_are_not_found(torch_cuda):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import chessboard, cv_hip
    rng = np.random.default_rng(3)
    blank = np.clip(np.rint(128 + 2.0 * rng.standard_normal((480, 640))), 0, 255).astype(np.uint8)
    frames = np.stack([blank, S.half_outside(), S.view("cam5", 2)[0]])
    found = chessboard.find_chessboard(torch.from_numpy(frames).cuda(), S.PATTERN)
    assert [f for f, _ in found] == [False, False, True] and not found[0][1].any() and not found[1][1].any()
    ok, corners = cv_hip.findChessboardCorners(frames[1], S.PATTERN)
    assert ok is False and corners.shape == (54, 1, 2) and corners.dtype == np.float32 and not corners.any()
    # the board is there, the pattern asked for is not
    assert not cv_hip.findChessboardCorners(frames[2], (8, 6))[0] and not cv_hip.findChessboardCorners(frames[2], (9, 5))[0]
    assert cv_hip.findChessboardCorners(frames[2], (6, 9))[0]


def test_cv_find_chessboard_corners_equals_find_chessboard(torch_cuda):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import chessboard, cv_hip
    frame, truth = S.view("cam5", 3, True)
    ok, corners = cv_hip.findChessboardCorners(frame, S.PATTERN, None, 0)
    (ok2, pts), = chessboard.find_chessboard(torch.from_numpy(np.array(frame)[None]).cuda(), S.PATTERN)
    assert ok is True and ok2 and corners.dtype == np.float32 and corners.shape == (54, 1, 2) and corners.reshape(54, 2).tobytes() == pts.tobytes()
    assert np.hypot(*(corners.reshape(54, 2) - truth).T).max() <= bound("cam5", True)[1] + 1e-6
    turned = cv_hip.findChessboardCorners(frame, (6, 9))[1].reshape(9, 6, 2)
    G = corners.reshape(6, 9, 2)
    assert any(np.array_equal(turned, t) for t in (G[::-1].transpose(1, 0, 2), G[:, ::-1].transpose(1, 0, 2))), "the same grid, turned"
    with pytest.raises(cv_hip.error, match="AGT_CHESS_ERR_ARG"):
        cv_hip.findChessboardCorners(frame, S.PATTERN, nms=0)
    with pytest.raises(cv_hip.error, match="unknown"):
        cv_hip.findChessboardCorners(frame, S.PATTERN, winSize=5)
    with pytest.raises(cv_hip.error, match="AGT_CHESS_ERR_ARG"):
        cv_hip.findChessboardCorners(np.array(frame)[:10], S.PATTERN)


def test_calibration_from_found_corners(torch_cuda):
    """calibrate_camera on the corners found in 12 noisy views: it converges, the held-out views reproject better with the calibrated
    camera than with the one the solve started from (the criterion of test_gpu_camera_calib.py::test_noisy_solve), and the final RMS is
    no more than 1.5 times the corner RMS of the class"""
    from accurate_aprilgroup_tracking_amd import camera_calib as cc, cv_hip
    views = S.calibration_views()
    obj, img, used = cc.target_points_from_chessboards([f for f, _ in views], S.PATTERN, S.PITCH)
    assert used == list(range(S.N_CAL + S.N_HELD)) and all(o.shape == (54, 3) and m.shape == (54, 2) for o, m in zip(obj, img))
    corner_rms = float(np.sqrt(np.mean([np.sum((m - t) ** 2, axis=1) for m, (_, t) in zip(img, views)])))
    rms, mtx, dist, rvecs, tvecs, rep = cc.calibrate_camera(obj[:S.N_CAL], img[:S.N_CAL], S.CLASSES["cam5"][1])
    err = {}
    for name, c in (("calibrated", rep["camera"]), ("start", rep["initial_camera"])):
        K, dc = cc.camera_from_vector(c, 5)
        e = []
        for v in range(S.N_CAL, S.N_CAL + S.N_HELD):
            ok, r, t = cv_hip.solvePnP(obj[v], img[v], K, dc)
            proj, _ = cv_hip.projectPoints(obj[v], r, t, K, dc)
            e.append(np.linalg.norm(proj.reshape(-1, 2) - img[v], axis=1).mean())
        err[name] = float(np.mean(e))
    print("corner RMS of the %d views %.4f px; calibration: %s after %d iterations, RMS %.4f px (bound %.4f); held-out mean reprojection error: calibrated %.4f px, start %.4f px"
          % (len(views), corner_rms, rep["stop_reason"], rep["iterations"], rms, 1.5 * MEASURED[("cam5", True)][0], err["calibrated"], err["start"]))
    print("camera: %s (truth %s)" % (np.array2string(rep["camera"][:9], precision=5), np.array2string(S.CLASSES["cam5"][0][:9], precision=5)))
    assert rep["stop_reason"] == "converged"
    assert err["calibrated"] < err["start"]
    assert rms <= 1.5 * MEASURED[("cam5", True)][0]


def test_tool_calibrates_from_a_stack_of_frames(torch_cuda, tmp_path, capsys):
    """tools/calibrate_camera.py --chessboard on an .npz stack (gray) and an .npy stack (BGR) of the calibration views, in this
    process: the file it writes holds the camera calibrate_camera gives on the same corners"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import calibrate_camera as tool
    from accurate_aprilgroup_tracking_amd import camera_calib as cc, formats
    frames = np.stack([f for f, _ in S.calibration_views()[:S.N_CAL]])
    np.savez(tmp_path / "gray.npz", frames=frames[:8])
    np.save(tmp_path / "bgr.npy", np.repeat(frames[8:, :, :, None], 3, axis=3))
    out = tmp_path / "CameraParams.npz"
    assert tool.main(["--chessboard", "9", "6", "--square", str(S.PITCH), str(tmp_path / "gray.npz"), str(tmp_path / "bgr.npy"), "-o", str(out)]) == 0
    text = capsys.readouterr().out
    assert "frames of the recording with the board: %d of %d" % (S.N_CAL, S.N_CAL) in text and "converged" in text
    mtx, dist, rvecs, tvecs = formats.load_camera_params(str(out))
    obj, img, _ = cc.target_points_from_chessboards(list(frames), S.PATTERN, S.PITCH)
    want = cc.calibrate_camera(obj, img, S.CLASSES["cam5"][1])
    assert np.array_equal(mtx, want[1]) and np.array_equal(np.ravel(dist), np.ravel(want[2])) and len(rvecs) == len(tvecs) == S.N_CAL


def test_draw_chessboard_corners_equals_overlay_numpy(torch_cuda):
    import overlay_numpy as on
    from accurate_aprilgroup_tracking_amd import cv_hip
    frame, truth = S.view("cam5", 0)
    corners = truth.reshape(-1, 1, 2).astype(np.float32)
    for found in (True, False):
        for img in (np.array(frame), np.repeat(np.array(frame)[:, :, None], 3, axis=2)):
            want = on.raster(img.copy(), cv_hip.chessboard_display_list(S.PATTERN, corners, found))
            got = cv_hip.drawChessboardCorners(img, S.PATTERN, corners, found)
            assert got is img and got.tobytes() == want.tobytes() and np.count_nonzero(got != (frame if img.ndim == 2 else frame[:, :, None])) > 54 * 20
