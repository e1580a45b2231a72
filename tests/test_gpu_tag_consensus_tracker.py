"""-m gpu: tag consensus in the tracker (agt_tracker_consensus) on the sliding-tags scene of tests/consensus_scenes.py -- the device state
machine against the stage-by-stage chain (the tracker's own LK corners -> the host rule with the CPU oracle -> agt_estimate_pose on a
second context with that mask; bitwise) and against the PoseDetector cv-backend mirror (the tolerance of tests/test_gpu_fb_check.py)."""
import ctypes as C

import numpy as np
import pytest

import consensus_scenes as S

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-8            # tests/test_gpu_fb_check.py, the same comparison


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def scene():
    return S.SlidingSequence()


def _download(trk):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    cp, sp = trk.corners()
    c = np.zeros((trk.B, trk.n, 2), np.float32); s = np.zeros((trk.B, trk.n), np.uint8)
    H.check(trk.ctx.L.agt_download(trk.ctx.h, c.ctypes.data_as(C.c_void_p), C.c_void_p(cp), c.nbytes), "agt_download")
    H.check(trk.ctx.L.agt_download(trk.ctx.h, s.ctypes.data_as(C.c_void_p), C.c_void_p(sp), s.nbytes), "agt_download")
    return c, s


def _tracker(torch, sc, k0=0, gate=False, depth=1, **kw):
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    trk = StreamTracker(sc.width, sc.height, sc.obj, sc.K, sc.dist, n_streams=1, **kw)
    if gate:
        trk.tag_gate(4)
    trk.pipeline(depth)
    f0 = torch.from_numpy(sc.frame(k0)[None]).cuda().contiguous()
    trk.reset(f0, torch.from_numpy(sc.corners(k0)[None].astype(np.float32)).cuda().contiguous())
    return trk


def run_records(torch, sc, many=False, prelude=None, gate=False, depth=1, **kw):
    """the whole scene through one tracker -> records [steps, 16], final corners, final status"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    trk = _tracker(torch, sc, gate=gate, depth=depth, **kw)
    steps = len(sc) - 1
    clip = torch.from_numpy(np.stack([sc.frame(k)[None] for k in range(1, steps + 1)])).cuda().contiguous()
    if prelude is not None:
        prelude(trk, clip)
        trk.reset(torch.from_numpy(sc.frame(0)[None]).cuda().contiguous(), torch.from_numpy(sc.corners(0)[None].astype(np.float32)).cuda().contiguous())
    so = torch.zeros((steps, 1, H.STATE_STRIDE), dtype=torch.float64, device="cuda")
    if many:
        trk.step_many(clip, so)
    else:
        for i in range(steps):
            trk.step(clip[i], so[i])
    trk.join()
    torch.cuda.synchronize()
    c, s = _download(trk)
    return so.cpu().numpy()[:, 0], c[0], s[0]


def chain_against_tracker(torch, oracle, sc, k0, steps, gate=False, depth=1, lk=None, skip_slots=(), **kw):
    """Lock step: the tracker with the option on; after each of its frames the chain -- its LK corners and status (lk: a callable that
    supplies them where the pose step's refresh overwrites the tracker's), the oracle's host rule from the second context's guess (with
    the margin condition), agt_estimate_pose on the second context with mask = status AND inliers.  -> the tracker's records."""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    trk = _tracker(torch, sc, k0, gate, depth, consensus_px=S.TAU, **kw)
    kw2 = {k: v for k, v in kw.items() if k != "fb_check"}
    ref = _tracker(torch, sc, k0, gate, 0, **kw2)
    obj32 = sc.obj.astype(np.float32)
    recs = []
    for i in range(steps):
        so = torch.zeros((1, H.STATE_STRIDE), dtype=torch.float64, device="cuda"); so2 = torch.zeros_like(so)
        trk.step(torch.from_numpy(sc.frame(k0 + 1 + i)[None]).cuda().contiguous(), so)
        trk.join()
        torch.cuda.synchronize()
        c, s = lk(i) if lk is not None else tuple(a[0] for a in _download(trk))
        st = ref.read_state()[0]
        guess = np.array(st.guess[:]) if st.has_guess else None
        usable = s != 0
        res = S.oracle_rule(oracle, obj32, c, sc.K, sc.dist, usable=usable, guess=guess)
        closest = S.check_margins(res, usable)
        mask = (usable & res["inliers"]).astype(np.uint8)
        ref.estimate_pose(torch.from_numpy(c[None].copy()).cuda().contiguous(), torch.from_numpy(mask[None]).cuda().contiguous(), so2)
        torch.cuda.synchronize()
        g, r = so.cpu().numpy()[0], so2.cpu().numpy()[0]
        where = "frame %d" % (k0 + 1 + i)
        print("%s: winner %d with %d inliers (closest residual %.3f px from the threshold), ok %d err %.3f ntrack %d" %
              (where, res["winner"], res["count"], closest, g[H.ST_OK], g[H.ST_ERR], g[H.ST_NTRACK]))
        keep = [j for j in range(H.STATE_STRIDE) if j != H.ST_NINLIER and j not in skip_slots]
        assert np.array_equal(g[keep].view(np.uint64), r[keep].view(np.uint64)), where + ": record %s, chain %s" % (g, r)
        assert g[H.ST_NINLIER] == res["count"] and r[H.ST_NINLIER] == 0.0, where
        recs.append((g, res, usable))
    return recs, trk


@pytest.mark.parametrize("depth", [0, 4])
def test_tracker_equals_the_stage_by_stage_chain(torch_cuda, oracle, scene, depth):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    recs, trk = chain_against_tracker(torch_cuda, oracle, scene, 0, len(scene) - 1, depth=depth)
    slid = np.zeros(48, bool)
    for t in S.OCC_TAGS:
        slid[4 * t:4 * t + 4] = True
    for k, (g, res, usable) in enumerate(recs, start=1):
        assert g[H.ST_OK] == 1.0 and usable.all(), "frame %d" % k            # LK keeps the slid corners: nothing else drops them
        assert g[H.ST_NTRACK] == res["count"]
        if k >= S.OCC_FROM:
            assert not res["inliers"][slid].all() and res["inliers"][~slid].all() and res["count"] < 48
    # not sticky: the status bytes still say 1 everywhere
    assert _download(trk)[1].all()


def test_tracker_equals_the_mirror_and_the_option_rescues_the_stream(torch_cuda, oracle, scene, tmp_path):
    """with the tag gate (the mirror solves on whole tags): records against PoseDetector(backend="cv", cv=oracle, pnp_consensus_px=2);
    the mirror accepts every frame with the option and rejects the covered ones without it, and so does the device"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    on = S.mirror_chain(oracle, scene, tmp_path, "on", S.TAU)
    off = S.mirror_chain(oracle, scene, tmp_path, "off", None)
    assert all(r["ok"] for r in on) and not all(r["ok"] for r in off)
    rec, c, s = run_records(torch_cuda, scene, gate=True, consensus_px=S.TAU)
    plain, _, _ = run_records(torch_cuda, scene, gate=True)
    for i, (r, p) in enumerate(zip(on, off)):
        g = rec[i]
        where = "frame %d" % (i + 1)
        assert bool(g[H.ST_OK]) == r["ok"] and bool(plain[i, H.ST_OK]) == p["ok"], where
        assert np.abs(g[:6] - r["pose"]).max() <= POSE_TOL, where + ": pose %g" % np.abs(g[:6] - r["pose"]).max()
        assert abs(g[H.ST_ERR] - r["err"]) < 1e-4 and bool(g[H.ST_GUESS]) == r["guided"] and g[H.ST_NINLIER] == r["consensus"][1], where
        assert plain[i, H.ST_NINLIER] == 0.0 and np.abs(plain[i, :6] - p["pose"]).max() <= POSE_TOL
    assert np.array_equal(c.view(np.uint32), on[-1]["pts"].view(np.uint32)) and np.array_equal(s.astype(bool), on[-1]["status"])
    truth = np.stack([scene.truth(k) for k in range(1, len(scene))])
    gap_on, gap_off = np.abs(rec[:, :6] - truth).max(axis=1), np.abs(plain[:, :6] - truth).max(axis=1)
    print("pose gap to truth: with the option %s, without %s; accepted %d / %d against %d / %d" %
          (gap_on, gap_off, rec[:, H.ST_OK].sum(), len(rec), plain[:, H.ST_OK].sum(), len(rec)))
    assert (gap_off[S.OCC_FROM - 1:] > 5 * gap_on[S.OCC_FROM - 1:]).all()


def test_clip_call_and_off_means_off(torch_cuda, scene):
    """agt_track_frames gives the per-frame records; consensus on for a few frames, then off and a reset: a tracker that never had it on"""
    rec, c, s = run_records(torch_cuda, scene, consensus_px=S.TAU)
    rec_m, c_m, s_m = run_records(torch_cuda, scene, many=True, consensus_px=S.TAU)
    assert np.array_equal(rec.view(np.uint64), rec_m.view(np.uint64)) and np.array_equal(c.view(np.uint32), c_m.view(np.uint32))

    def prelude(trk, clip):
        trk.consensus(S.TAU)
        for f in clip[:2]:
            trk.step(f)
        trk.consensus(0)
    for depth in (0, 1):
        fresh = run_records(torch_cuda, scene, depth=depth)
        again = run_records(torch_cuda, scene, depth=depth, prelude=prelude)
        assert np.array_equal(fresh[0].view(np.uint64), again[0].view(np.uint64)), "records, depth %d" % depth
        assert np.array_equal(fresh[1].view(np.uint32), again[1].view(np.uint32)) and np.array_equal(fresh[2], again[2])
        assert (fresh[0][:, 14] == 0.0).all()


@pytest.mark.parametrize("what", ["fb_check", "tag_gate", "reproject_view"])
def test_composition_one_frame(torch_cuda, oracle, scene, what):
    """one frame each, from frame OCC_FROM - 1 into the first covered frame: the option with fb_check, with the tag gate, and with
    reproject + the visibility rule (whose refresh overwrites the tracker's corners: the chain's LK is the oracle's, bit-exact)"""
    import fb_scenes
    from accurate_aprilgroup_tracking_amd import hiplib as H
    k0 = S.OCC_FROM - 1
    a, b, p0 = scene.frame(k0), scene.frame(k0 + 1), scene.corners(k0).astype(np.float32)
    if what == "fb_check":
        recs, trk = chain_against_tracker(torch_cuda, oracle, scene, k0, 1, fb_check=1.0)
        nx, st, _, _, _ = fb_scenes.oracle_fb(oracle, a, b, p0, 1.0)
        c, s = _download(trk)
        assert np.array_equal(s[0], st) and np.array_equal(c[0].view(np.uint32), nx.astype(np.float32).view(np.uint32)) and not st.all()
    elif what == "tag_gate":
        recs, trk = chain_against_tracker(torch_cuda, oracle, scene, k0, 1, gate=True)
        g, res, usable = recs[0]
        assert g[H.ST_NTRACK] == 4 * res["inliers"].reshape(-1, 4).all(axis=1).sum() and g[H.ST_NTRACK] <= res["count"]
    else:
        nx, st, _ = oracle.calcOpticalFlowPyrLK(a, b, p0, winSize=(21, 21), maxLevel=2)
        lk = lambda i: (nx.reshape(-1, 2).astype(np.float32), st.ravel().astype(np.uint8))
        recs, trk = chain_against_tracker(torch_cuda, oracle, scene, k0, 1, lk=lk, skip_slots=(H.ST_NVISIBLE,), reproject=True, view_deg=80.0)
        g, res, usable = recs[0]
        c, s = _download(trk)
        assert g[H.ST_OK] == 1.0 and 0 < g[H.ST_NVISIBLE] <= 12 and s[0].sum() == 4 * g[H.ST_NVISIBLE]
        proj = oracle.projectPoints(scene.obj.astype(np.float64), g[:3], g[3:6], scene.K, scene.dist)[0].reshape(-1, 2)
        assert np.abs(c[0] - proj).max() < 1e-3                 # the refresh ran on the consensus pose: every corner back on the body
    g, res, usable = recs[0]
    assert g[H.ST_OK] == 1.0 and res["count"] < usable.sum(), "the covered tags were not outvoted"


def test_dense_frames_are_refused_and_arguments(torch_cuda, scene):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    torch = torch_cuda
    trk = _tracker(torch, scene, consensus_px=S.TAU)
    f1 = torch.from_numpy(scene.frame(1)[None]).cuda().contiguous()
    for call in (lambda: trk.step_dense(f1), lambda: trk.step_many_dense(f1[None])):
        with pytest.raises(H.AgtError) as e:
            call()
        assert e.value.code == -6                      # AGT_ERR_UNSUPPORTED
    trk.consensus(0)
    with pytest.raises(H.AgtError) as e:
        trk.step_dense(f1)
    assert e.value.code == -7                          # AGT_ERR_STATE: no dense model -- the refusal above was the option's
    for args in ((-1.0, 4, 8), (float("nan"), 4, 8), (float("inf"), 4, 8), (2.0, 3, 8), (2.0, 4, 3), (2.0, 5, 8)):
        with pytest.raises(H.AgtError) as e:
            trk.consensus(*args)
        assert e.value.code == -1, args


@pytest.mark.parametrize("one_call", [False, True], ids=["detector_present", "one_call_path"])
def test_pose_detector_stream_loop(tmp_path, oracle, scene, torch_cuda, one_call):
    """PoseDetector(backend="stream", pnp_consensus_px=2) against the cv-backend mirror with the same option and detections: the
    detector-fed first frame (agt_track_frame_detected), then LK frames (agt_track_frame, or agt_track_host_frame without a detector)"""
    import logging
    from oracle import cv2_shim
    from accurate_aprilgroup_tracking_amd import formats
    log = logging.getLogger("test"); log.setLevel(logging.CRITICAL)

    class First:
        def __init__(self):
            self.k = 0

        def __call__(self, gray):
            self.k += 1
            if self.k > 1:
                return []
            c = scene.corners(0).reshape(-1, 4, 2)
            return [formats.make_detection(int(t), c[i], decision_margin=75.0) for i, t in enumerate(scene.group["tags"].keys())]
    Det = S.detector_class(tmp_path, scene, "pd")
    ref = Det(log, scene.K, None, True, cv=cv2_shim.make_cv2(), detector=First(), pnp_consensus_px=S.TAU)
    hip = Det(log, scene.K, None, True, detector=First(), backend="stream", pnp_consensus_px=S.TAU)
    vec = lambda p: None if p[0] is None else np.concatenate([np.asarray(p[0], np.float64).ravel(), np.asarray(p[1], np.float64).ravel()])
    for k in range(len(scene)):
        for d in (ref, hip):
            d._detect_and_get_pose(scene.frame(k))
            if one_call and k == 0:
                d.detector = None
        where = "frame %d" % k
        assert np.abs(vec(hip.last_pose) - vec(ref.last_pose)).max() <= POSE_TOL, where
        assert abs(hip.last_error - ref.last_error) < 1e-4 and ref.last_error < 2, where
        for x, y in ((hip.extrinsic_guess, ref.extrinsic_guess), (hip.prev_transform, ref.prev_transform)):
            assert (vec(x) is None) == (vec(y) is None) and (vec(x) is None or np.abs(vec(x) - vec(y)).max() <= POSE_TOL), where
