"""-m gpu: the forward-backward check of LK tracks at its three levels -- agt_lk_track_fb, the tracker option, the PoseDetector loop.

Expected values always come from two `oracle.calcOpticalFlowPyrLK` calls and the float32 rule of include/agt_hip.h
(tests/fb_scenes.py oracle_fb); the scenes and what makes them worth testing on are checked on the CPU in tests/test_fb_check.py.
agt_track_frame_dense with the check on is REFUSED (AGT_ERR_UNSUPPORTED): test_dense_frames_are_refused_while_the_check_is_on.
"""
import ctypes as C
import json
import logging

import numpy as np
import pytest

import fb_scenes as S

pytestmark = pytest.mark.gpu
LOG = logging.getLogger("test"); LOG.setLevel(logging.CRITICAL)
POSE_TOL = 1e-8


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


@pytest.fixture(scope="module")
def cvh(torch_cuda):
    from accurate_aprilgroup_tracking_amd import cv_hip
    return cv_hip


@pytest.fixture(scope="module")
def scene720():
    return S.OccludedSequence(*S.SCENE_720P)


@pytest.fixture(scope="module")
def scene480():
    return S.OccludedSequence(*S.SCENE_480P)


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _win_pair(win):
    return (win, win) if isinstance(win, int) else tuple(win)


def _extra_points(w, h, seed, n_random=24):
    """border and outside points, and points off the tags (the background is textured: some track, some do not)"""
    rng = np.random.default_rng(seed)
    edge = np.array([[0.0, 0.0], [w - 1.0, h - 1.0], [-5.5, 10.25], [w + 3.0, 7.0], [3.2, h + 8.9], [-40.0, -40.0],
                     [w + 30.0, h + 30.0], [10.5, 10.5], [w - 11.0, h - 11.0], [1.0, h / 2.0]], np.float32)
    return np.concatenate([edge, rng.uniform([-15, -15], [w + 15, h + 15], size=(n_random, 2)).astype(np.float32)])


class Pair:
    """B frame pairs on the device in a context of their own: agt_lk_track and agt_lk_track_fb on the same inputs"""

    def __init__(self, cvh, torch, frames_a, frames_b, n, win=21, max_level=2):
        self.torch = torch
        B, h, w = frames_a.shape
        ww, wh = _win_pair(win)
        self.ctx = cvh.Context(w, h, max_level=max_level, win=ww if ww == wh else (ww | (wh << 8)), max_points=n, max_streams=B)
        self.fa = torch.from_numpy(np.ascontiguousarray(frames_a)).cuda().contiguous()
        self.fb = torch.from_numpy(np.ascontiguousarray(frames_b)).cuda().contiguous()
        self.ctx.pyramid_build(0, self.fa); self.ctx.pyramid_build(1, self.fb)

    def run(self, pts, fb_px, next_pts=None, flags=0):
        torch = self.torch
        pg = torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float32)).cuda().contiguous()

        def init():
            return None if next_pts is None else torch.from_numpy(np.ascontiguousarray(next_pts, dtype=np.float32)).cuda().contiguous()
        plain = self.ctx.lk_track(0, 1, pg, init(), flags=flags)
        chk = self.ctx.lk_track_fb(0, 1, pg, init(), flags=flags, fb_threshold=fb_px)
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in plain], [x.cpu().numpy() for x in chk]


def _assert_stream(oracle, a, b, pts, plain, chk, bidx, fb_px, win=21, max_level=2, next_pts=None, flags=0, what=""):
    """stream bidx of a launch against the oracle composition on its own frame pair"""
    nx, st, er, dist, st_f = S.oracle_fb(oracle, a, b, pts, fb_px, win=_win_pair(win), max_level=max_level, flags=flags, next_pts=next_pts)
    where = "%s stream %d" % (what, bidx)
    assert np.array_equal(plain[1][bidx], st_f), where + ": agt_lk_track status against the oracle"
    for k, name in ((0, "next_pts"), (2, "err")):
        assert np.array_equal(_u32(chk[k][bidx]), _u32(plain[k][bidx])), where + ": %s differs from agt_lk_track" % name
    assert np.array_equal(_u32(chk[0][bidx]), _u32(nx)), where + ": next_pts against the oracle"
    assert np.array_equal(_u32(chk[2][bidx]), _u32(er)), where + ": err against the oracle"
    assert np.array_equal(chk[1][bidx], st), where + ": status; got %s, oracle %s" % (np.nonzero(chk[1][bidx] != st)[0], st[chk[1][bidx] != st])
    assert np.array_equal(_u32(chk[3][bidx]), _u32(dist)), where + ": fb_dist, max diff %g" % np.nanmax(np.abs(chk[3][bidx] - dist))
    return st, st_f, dist


@pytest.mark.parametrize("size", ["480p", "720p", "1080p"])
def test_lk_track_fb_four_waves_per_corner(torch_cuda, cvh, oracle, scene480, scene720, seq1080, size):
    """one stream (<= 1024 corners: four waves per corner, row-segment and general bodies), pyramid depths 0-3, thresholds 0.5 / 1 / 4,
    forward USE_INITIAL_FLOW, border and outside points; 480p and 720p: the pair in which the occluder appears"""
    if size == "1080p":
        a, b, base = seq1080.frame(0), seq1080.frame(1), seq1080.corners(0)
    else:
        sc = scene480 if size == "480p" else scene720
        a, b, base = sc.frame(S.OCC_FROM - 1), sc.frame(S.OCC_FROM), sc.corners(S.OCC_FROM - 1)
    h, w = a.shape
    pts = np.concatenate([base, _extra_points(w, h, 3)]).astype(np.float32)
    n = pts.shape[0]
    assert n <= 1024
    init = (pts + np.random.default_rng(4).normal(0, 1.5, pts.shape)).astype(np.float32)
    kept = {}
    for ml in (0, 1, 2, 3):
        pair = Pair(cvh, torch_cuda, a[None], b[None], n, max_level=ml)
        variants = [dict(fb_px=1.0)] if ml != 2 else [dict(fb_px=1.0), dict(fb_px=0.5), dict(fb_px=4.0), dict(fb_px=1.0, flags=4, next_pts=init)]
        for kw in variants:
            nxt = kw.get("next_pts")
            plain, chk = pair.run(pts[None], kw["fb_px"], None if nxt is None else nxt[None], kw.get("flags", 0))
            st, st_f, dist = _assert_stream(oracle, a, b, pts, plain, chk, 0, kw["fb_px"], max_level=ml, next_pts=nxt,
                                            flags=kw.get("flags", 0), what="%s level %d %r" % (size, ml, sorted(kw)))
            if ml == 2 and "flags" not in kw:
                kept[kw["fb_px"]] = int(st.sum())
                if kw["fb_px"] == 1.0 and size != "1080p":
                    assert st_f[:4].all() and st[:4].sum() <= 1, "the occluded corners pass plain LK and fail the check"
                    assert st[4:48].all(), "no clean corner is dropped"
                assert (dist[st_f == 0] == -1.0).all() and (st_f == 0).any()
    assert kept[0.5] <= kept[1.0] <= kept[4.0]


def test_lk_track_fb_one_wave_per_corner_distinct_streams(torch_cuda, cvh, oracle, scene480):
    """more than 1024 corners in the launch (one wave per corner, both of its bodies): B distinct frame pairs, the occluder on one of
    them; forward USE_INITIAL_FLOW; agt_lk_occupancy_cu caps change no bit"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    sc = scene480
    B, occ = 20, 5
    ks = [(b % 4, b % 4 + 1 + (b // 4) % 2) for b in range(B)]          # frame pairs (k0 -> k1), 1- and 2-frame gaps
    ks[occ] = (S.OCC_FROM - 1, S.OCC_FROM)
    fa = np.stack([sc.seq.frame(k0) for k0, _ in ks])                   # (every stream but `occ`: the clean frames)
    fb = np.stack([sc.frame(k1) if b == occ else sc.seq.frame(k1) for b, (_, k1) in enumerate(ks)])
    extra = _extra_points(sc.width, sc.height, 7, n_random=6)
    pts = np.stack([np.concatenate([sc.corners(k0), extra + 0.37 * b]) for b, (k0, _) in enumerate(ks)]).astype(np.float32)
    n = pts.shape[1]
    assert n * B > 1024
    init = (pts + np.random.default_rng(5).normal(0, 1.5, pts.shape)).astype(np.float32)
    pair = Pair(cvh, torch_cuda, fa, fb, n)
    ref = None
    for kw in (dict(), dict(flags=4, next_pts=init)):
        plain, chk = pair.run(pts, 1.0, kw.get("next_pts"), kw.get("flags", 0))
        for b in range(B):
            st, st_f, _ = _assert_stream(oracle, fa[b], fb[b], pts[b], plain, chk, b, 1.0, flags=kw.get("flags", 0),
                                         next_pts=None if "next_pts" not in kw else init[b], what="one wave %r" % sorted(kw))
            if not kw:
                if b == occ:
                    assert st_f[:4].all() and st[:4].sum() <= 1, "the occluded stream loses its occluded corners"
                else:
                    assert st[:48].sum() >= 46, "stream %d is clean" % b
        if not kw:
            ref = chk
    for cap in (10, 1, 5, -1):
        H.check(pair.ctx.L.agt_lk_occupancy_cu(pair.ctx.h, cap), "agt_lk_occupancy_cu")
        _, chk = pair.run(pts, 1.0)
        assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(ref, chk)), "cap %d per CU" % cap


@pytest.mark.parametrize("win", [15, 31, (13, 13), (17, 11)], ids=["15", "31", "13x13", "17x11"])
def test_lk_track_fb_other_windows(torch_cuda, cvh, oracle, scene480, win):
    """the other compiled-in windows (one wave per corner) and two windows of the general body: the occluder pair"""
    sc = scene480
    a, b = sc.frame(S.OCC_FROM - 1), sc.frame(S.OCC_FROM)
    pts = np.concatenate([sc.corners(S.OCC_FROM - 1), _extra_points(sc.width, sc.height, 9)]).astype(np.float32)
    pair = Pair(cvh, torch_cuda, a[None], b[None], pts.shape[0], win=win)
    for fb_px in (1.0, 0.5):
        plain, chk = pair.run(pts[None], fb_px)
        st, st_f, _ = _assert_stream(oracle, a, b, pts, plain, chk, 0, fb_px, win=win, what="window %r" % (win,))
    assert st_f[:48].sum() > st[:48].sum() >= 24


def test_track_forward_backward_cv_call(cvh, oracle, scene720):
    """cv_hip.trackForwardBackward: the numpy-in / numpy-out form, and its argument check"""
    sc = scene720
    a, b, pts = sc.frame(S.OCC_FROM - 1), sc.frame(S.OCC_FROM), sc.corners(S.OCC_FROM - 1)
    nx, st, er, fd = cvh.trackForwardBackward(a, b, pts, winSize=(21, 21), maxLevel=2)
    enx, est, eer, edist, _ = S.oracle_fb(oracle, a, b, pts)
    assert nx.shape == (48, 1, 2) and st.shape == er.shape == fd.shape == (48, 1)
    assert np.array_equal(_u32(nx.reshape(-1, 2)), _u32(enx)) and np.array_equal(st.ravel(), est)
    assert np.array_equal(_u32(er.ravel()), _u32(eer)) and np.array_equal(_u32(fd.ravel()), _u32(edist))
    assert est.sum() == 44 and not est[:4].any()
    gnx, gst, ger = cvh.calcOpticalFlowPyrLK(a, b, pts, None, winSize=(21, 21), maxLevel=2)
    assert np.array_equal(_u32(gnx), _u32(nx)) and np.array_equal(_u32(ger), _u32(er)) and gst.all()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(cvh.error):
            cvh.trackForwardBackward(a, b, pts, fbThreshold=bad)


# ---------------------------------------------------------------------------------------------------------------- tracker
def _detector_class(tmp_path, sc, tag):
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    d = tmp_path / ("g_%s" % tag)
    d.mkdir(exist_ok=True)
    (d / "april_group.json").write_text(json.dumps(sc.group))

    class Det(PoseDetector):
        DIRPATH = str(d)
    return Det


def cpu_chain(oracle, sc, tmp_path, tag, fb_px=None, gate=False):
    """The stream's own CPU chain, after cpu_chain of tests/test_gpu_hetero.py, with the check (fb_px) and the tag gate added
    -> (records, final points, final status).  A corner the check drops is a corner LK lost in that frame."""
    from oracle import cv2_shim
    det = _detector_class(tmp_path, sc, tag)(LOG, sc.K, sc.dist, True, cv=cv2_shim.make_cv2())
    obj32 = sc.obj.astype(np.float32)
    n = obj32.shape[0]
    pts = sc.corners(0).astype(np.float32).copy(); alive = np.ones(n, bool)
    pyr = oracle.Pyramid(sc.frame(0), S.WIN, S.MAX_LEVEL)
    recs = []
    for k in range(1, len(sc)):
        npyr = oracle.Pyramid(sc.frame(k), S.WIN, S.MAX_LEVEL)
        if fb_px:
            nx, status, _, _, _ = S.oracle_fb(oracle, pyr, npyr, pts, fb_px, alive=alive)
        else:
            nx, status, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, winSize=(S.WIN, S.WIN), maxLevel=S.MAX_LEVEL)
            nx = nx.reshape(-1, 2); nx[~alive] = pts[~alive]
        alive = alive & status.ravel().astype(bool)
        use = np.repeat(alive.reshape(-1, 4).all(axis=1), 4) if gate else alive
        il = [nx[j].reshape(1, 1, 2) for j in range(n) if use[j]]
        ol = [obj32[j].reshape(1, 3) for j in range(n) if use[j]]
        guided = det.extrinsic_guess[0] is not None
        det._estimate_pose(il if len(il) >= 8 else [], ol if len(il) >= 8 else [])
        solved = det.last_error is not None
        recs.append(dict(ntrack=int(use.sum()), too_few=len(il) < 8, ok=bool(solved and det.last_error < 2),
                         guided=bool(guided and solved), err=det.last_error,
                         pose=None if not solved else np.concatenate([det.last_pose[0].ravel(), det.last_pose[1].ravel()]).astype(np.float64)))
        pts = nx.astype(np.float32); pyr = npyr
    return recs, pts, alive


def run_device(scs, depth, fb_px=0.0, gate=False, prelude=None):
    """all streams through ONE StreamTracker -> (records [steps, B, 16], corners [B, n, 2], status [B, n]).
    prelude(trk, frames): called after the first reset; the run proper starts with a second reset."""
    import torch
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    B, s0 = len(scs), scs[0]
    n, steps = s0.obj.shape[0], len(s0) - 1
    frames = [torch.from_numpy(np.stack([sc.frame(k) for sc in scs])).cuda().contiguous() for k in range(steps + 1)]
    c0 = torch.from_numpy(np.stack([sc.corners(0) for sc in scs]).astype(np.float32)).cuda().contiguous()
    trk = StreamTracker(s0.width, s0.height, s0.obj, s0.K, s0.dist, n_streams=B, fb_check=fb_px)
    if gate:
        trk.tag_gate(4)
    trk.pipeline(depth)
    trk.reset(frames[0], c0)
    if prelude is not None:
        prelude(trk, frames)
        trk.reset(frames[0], c0)
    so = torch.zeros((steps, B, H.STATE_STRIDE), dtype=torch.float64, device="cuda")
    for i in range(steps):
        trk.step(frames[i + 1], so[i])
    trk.join()
    torch.cuda.synchronize()
    rec = so.cpu().numpy()
    cp, sp = trk.corners()
    got_c = np.zeros((B, n, 2), np.float32); got_s = np.zeros((B, n), np.uint8)
    H.check(trk.ctx.L.agt_download(trk.ctx.h, got_c.ctypes.data_as(C.c_void_p), C.c_void_p(cp), got_c.nbytes), "agt_download")
    H.check(trk.ctx.L.agt_download(trk.ctx.h, got_s.ctypes.data_as(C.c_void_p), C.c_void_p(sp), got_s.nbytes), "agt_download")
    assert not (rec[:, :, H.ST_FLAGS].astype(int) & H.TRK_CHAIN_TIMEOUT).any()
    return rec, got_c, got_s


def compare(rec, got_c, got_s, chains):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    for b, (recs, pts, alive) in enumerate(chains):
        for i, r in enumerate(recs):
            g = rec[i, b]
            where = "stream %d step %d" % (b, i)
            assert int(g[H.ST_NTRACK]) == r["ntrack"], where + ": tracked corners %d, chain %d" % (g[H.ST_NTRACK], r["ntrack"])
            assert bool(int(g[H.ST_FLAGS]) & H.PNP_TOO_FEW) == r["too_few"], where + ": too-few flag"
            assert bool(g[H.ST_OK]) == r["ok"], where + ": acceptance"
            if r["pose"] is not None:
                assert np.abs(g[:6] - r["pose"]).max() <= POSE_TOL, where + ": pose %g" % np.abs(g[:6] - r["pose"]).max()
                assert bool(g[H.ST_GUESS]) == r["guided"], where + ": guess use"
        assert np.array_equal(got_s[b].astype(bool), alive), "stream %d: final status" % b
        assert np.array_equal(got_c[b].view(np.uint32), pts.view(np.uint32)), "stream %d: final corners" % b


def _streams(B, scene720):
    if B == 1:
        return [scene720]
    # three distinct streams of the same object, the occluder on stream 1
    w, h, seed = S.SCENE_720P
    return [S.OccludedSequence(w, h, 11, occluded=False, group_seed=seed), scene720, S.OccludedSequence(w, h, 12, occluded=False, group_seed=seed)]


@pytest.mark.parametrize("gate", [False, True], ids=["no_gate", "tag_gate"])
@pytest.mark.parametrize("B", [1, 3])
def test_tracker_with_the_check_matches_its_cpu_chain(oracle, tmp_path, scene720, B, gate):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    scs = _streams(B, scene720)
    occ = 0 if B == 1 else 1
    chains = [cpu_chain(oracle, sc, tmp_path, "fb%d_%d" % (B, b), fb_px=1.0, gate=gate) for b, sc in enumerate(scs)]
    rec0, c0, s0 = run_device(scs, 0, 1.0, gate)
    compare(rec0, c0, s0, chains)
    rec4, c4, s4 = run_device(scs, 4, 1.0, gate)
    assert np.array_equal(rec4.view(np.uint64), rec0.view(np.uint64)), "depth 4 against depth 0: records"
    assert np.array_equal(c4.view(np.uint32), c0.view(np.uint32)) and np.array_equal(s4, s0)
    # the scene did its work: only the occluded stream loses corners, and exactly tag 0's
    for b in range(B):
        want = np.ones(48, bool)
        if b == occ:
            want[:4] = False
        assert np.array_equal(s0[b].astype(bool), want), "stream %d: status %s" % (b, np.nonzero(s0[b] == 0)[0])
    assert (rec0[S.OCC_FROM - 1:, occ, H.ST_NTRACK] == 44).all() and (rec0[:, :, H.ST_OK] == 1).all()


def test_the_check_rescues_the_occluded_stream(oracle, tmp_path, scene720):
    """What the check is for, on the 720p scene: without it frames 2-5 are rejected by the reprojection gate (48 corners, four of them
    wrong); with it they are accepted on 44 corners and the poses are at least ten times closer to the scene's true trajectory."""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    plain, cp, sp = run_device([scene720], 0, 0.0)
    chk, _, _ = run_device([scene720], 0, 1.0)
    compare(plain, cp, sp, [cpu_chain(oracle, scene720, tmp_path, "plain")])
    fr = slice(S.OCC_FROM - 1, None)                       # records of frames 2 .. 5 (record i is frame i + 1)
    assert sp.all() and (plain[fr, 0, H.ST_NTRACK] == 48).all()
    assert (plain[fr, 0, H.ST_OK] == 0).all(), "the plain tracker accepts an occluded frame: %s" % plain[fr, 0, H.ST_ERR]
    assert (chk[fr, 0, H.ST_OK] == 1).all() and (chk[fr, 0, H.ST_NTRACK] == 44).all()
    truth = np.stack([scene720.truth(k) for k in range(1, len(scene720))])
    gap_plain = np.abs(plain[fr, 0, :6] - truth[fr]).max(axis=1)
    gap_chk = np.abs(chk[fr, 0, :6] - truth[fr]).max(axis=1)
    print("pose gap to truth, frames 2-5: plain %s checked %s; reprojection error plain %s checked %s"
          % (gap_plain, gap_chk, plain[fr, 0, H.ST_ERR], chk[fr, 0, H.ST_ERR]))
    assert (gap_plain >= 10.0 * gap_chk).all(), "plain %s, checked %s" % (gap_plain, gap_chk)


@pytest.mark.parametrize("depth", [0, 8])
def test_off_means_off(scene720, depth):
    """fb_check(1.0), a few frames, fb_check(0) and a reset: records and corners of a tracker that never had the check on"""
    def prelude(trk, frames):
        trk.fb_check(1.0)
        for f in frames[1:4]:
            trk.step(f)
        trk.fb_check(0)
    fresh = run_device([scene720], depth, 0.0)
    again = run_device([scene720], depth, 0.0, prelude=prelude)
    assert np.array_equal(fresh[0].view(np.uint64), again[0].view(np.uint64)), "records"
    assert np.array_equal(fresh[1].view(np.uint32), again[1].view(np.uint32)) and np.array_equal(fresh[2], again[2])
    assert fresh[2].all(), "the plain tracker keeps the occluded corners"


def test_dense_frames_are_refused_while_the_check_is_on(torch_cuda, scene720):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    torch = torch_cuda
    sc = scene720
    trk = StreamTracker(sc.width, sc.height, sc.obj, sc.K, None, fb_check=1.0)
    f0 = torch.from_numpy(sc.frame(0)[None]).cuda().contiguous(); f1 = torch.from_numpy(sc.frame(1)[None]).cuda().contiguous()
    trk.reset(f0, torch.from_numpy(sc.corners(0)[None]).cuda().contiguous())
    for call in (lambda: trk.step_dense(f1), lambda: trk.step_many_dense(f1[None])):
        with pytest.raises(H.AgtError) as e:
            call()
        assert e.value.code == -6                      # AGT_ERR_UNSUPPORTED
    trk.fb_check(0)
    with pytest.raises(H.AgtError) as e:
        trk.step_dense(f1)
    assert e.value.code == -7                          # AGT_ERR_STATE: no dense model -- the refusal above was the check's
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(H.AgtError):
            trk.fb_check(bad)


# ---------------------------------------------------------------------------------------------------------------- PoseDetector
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


def _vec(pair):
    return None if pair[0] is None else np.concatenate([np.asarray(pair[0], np.float64).ravel(), np.asarray(pair[1], np.float64).ravel()])


def _same_pair(a, b, what):
    va, vb = _vec(a), _vec(b)
    assert (va is None) == (vb is None), "%s: presence differs" % what
    if va is not None:
        assert np.abs(va - vb).max() <= POSE_TOL, "%s differs by %g" % (what, np.abs(va - vb).max())


@pytest.mark.parametrize("one_call", [False, True], ids=["detector_present", "one_call_path"])
def test_pose_detector_stream_loop_with_the_check(tmp_path, oracle, scene720, one_call):
    """PoseDetector(backend="stream", lk_fb_px=1.0) over the occluded stream against the oracle-backend mirror with the same option
    and the same detections, the state after every frame; one_call: without a detector after the first frame, the LK frames go
    through agt_track_host_frame"""
    from oracle import cv2_shim
    sc = scene720
    Det = _detector_class(tmp_path, sc, "pd")
    ref = Det(LOG, sc.K, None, True, cv=cv2_shim.make_cv2(), detector=FirstFrameDetector(sc), lk_fb_px=1.0)
    plain = Det(LOG, sc.K, None, True, cv=cv2_shim.make_cv2(), detector=FirstFrameDetector(sc))
    hip = Det(LOG, sc.K, None, True, detector=FirstFrameDetector(sc), backend="stream", lk_fb_px=1.0)
    for k in range(len(sc)):
        frame = sc.frame(k)
        for d in (ref, plain, hip):
            d._detect_and_get_pose(frame)
            if one_call and k == 0:
                d.detector = None
        where = "frame %d" % k
        _same_pair(hip.last_pose, ref.last_pose, where + " pose")
        assert (hip.last_error is None) == (ref.last_error is None)
        assert abs(hip.last_error - ref.last_error) < 1e-4 and (hip.last_error < 2) == (ref.last_error < 2)
        _same_pair(hip.extrinsic_guess, ref.extrinsic_guess, where + " guess")
        _same_pair(hip.prev_transform, ref.prev_transform, where + " prev_transform")
        assert len(hip.rot_velocities) == len(ref.rot_velocities)
        for x, y in zip(hip.rot_velocities + hip.tran_velocities, ref.rot_velocities + ref.tran_velocities):
            assert np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).max() <= POSE_TOL
        assert ref.last_error < 2, where + ": the checked mirror is gated out"
        if k >= S.OCC_FROM:
            assert len(ref._prev_ids) == 11 and plain.last_error >= 2, where + ": the plain mirror accepts the occluded frame"
