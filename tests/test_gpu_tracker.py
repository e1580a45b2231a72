"""-m gpu: the device-resident _estimate_pose state machine and the fused per-frame step.

  * agt_estimate_pose vs the fixtures produced by the REFERENCE's own Python state machine
  * the PoseDetector mirror running on the HIP backend vs the same fixtures
  * agt_track_frame (pyramid + LK + PnP + motion model, no host round trip) vs the same chain
    assembled from oracle pieces
Tolerance: POSE_TOL on poses/guesses (north_star bound 1e-4); LK corners bit-exact.
"""
import json
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
POSE_TOL = 1e-8
LOG = logging.getLogger("test"); LOG.setLevel(logging.CRITICAL)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("name", ["reference_state_machine_enhanced.npz", "reference_state_machine_plain.npz"])
def test_device_state_machine_matches_reference(torch_cuda, name):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    fx = np.load(os.path.join(GOLD, name))
    F, T = fx["tagmask"].shape
    B = 3                                    # same stream replicated: exercises batching
    trk = StreamTracker(1280, 720, fx["all_objpts"], fx["K"], fx["dist"], n_streams=B,
                        enhance_ape=bool(int(fx["enhance_ape"])))
    trk.reset()
    so = trk.new_state_buffer()
    for k in range(F):
        img = torch.from_numpy(np.repeat(fx["corners"][k][None].astype(np.float32), B, 0)).cuda().contiguous()
        mask = torch.from_numpy(np.repeat(np.repeat(fx["tagmask"][k], 4)[None].astype(np.uint8), B, 0)).cuda().contiguous()
        trk.estimate_pose(img, mask, so)
        st = so.cpu().numpy()
        states = trk.read_state()
        for b in range(B):
            ok = int(st[b, H.ST_OK])
            assert ok == fx["pose_valid"][k], "frame %d acceptance" % k
            if ok:
                assert np.abs(st[b, :6] - fx["pose"][k]).max() < POSE_TOL, "frame %d pose" % k
                assert int(st[b, H.ST_TVEC_F32]) == fx["tvec_f32"][k]
            s = states[b]
            assert s.has_guess == fx["guess_valid"][k], "frame %d guess presence" % k
            if s.has_guess:
                assert np.abs(np.array(s.guess[:]) - fx["guess"][k]).max() < POSE_TOL, "frame %d guess" % k
                assert s.guess_t_f32 == fx["guess_t_f32"][k]
            assert s.n_vel == fx["n_vel"][k]
            for i in range(s.n_vel):
                assert np.abs(np.array(s.rot_vel[i][:]) - fx["rot_vel"][k][i]).max() < POSE_TOL
                assert np.abs(np.array(s.tran_vel[i][:]) - fx["tran_vel"][k][i]).max() < POSE_TOL
            if fx["prev_valid"][k]:
                assert s.has_prev and np.abs(np.array(s.prev[:]) - fx["prev"][k]).max() < POSE_TOL


@pytest.mark.parametrize("name", ["reference_state_machine_enhanced.npz"])
def test_pose_detector_mirror_on_hip_backend(tmp_path, name):
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    fx = np.load(os.path.join(GOLD, name))
    (tmp_path / "april_group.json").write_text(json.dumps(json.loads(str(fx["group_json"]))))

    class Det(PoseDetector):
        DIRPATH = str(tmp_path)
    det = Det(LOG, fx["K"], fx["dist"], bool(int(fx["enhance_ape"])))      # default backend = cv_hip
    assert det.cv.__name__.endswith("cv_hip")
    tag_ids = sorted(det.extrinsics)
    F, T = fx["tagmask"].shape
    for k in range(F):
        img_list, obj_list = [], []
        for t, tid in enumerate(tag_ids):
            if fx["tagmask"][k, t]:
                size, tvec, rvec = det.extrinsics[tid][:3]
                img_list.append(fx["corners"][k, 4 * t:4 * t + 4].reshape(1, 4, 2))
                obj_list.append(det.transform_marker_corners(det.get_initial_pts(size), (rvec, tvec)))
        before = det.prev_transform
        det._estimate_pose(img_list, obj_list)
        accepted = det.prev_transform is not before
        assert int(accepted) == fx["pose_valid"][k]
        if accepted:
            pose = np.concatenate([det.prev_transform[0].ravel(), det.prev_transform[1].ravel()]).astype(np.float64)
            assert np.abs(pose - fx["pose"][k]).max() < POSE_TOL
            assert int(det.prev_transform[1].dtype == np.float32) == fx["tvec_f32"][k]
        if det.extrinsic_guess[0] is not None:
            g = np.concatenate([det.extrinsic_guess[0].ravel(), det.extrinsic_guess[1].ravel()]).astype(np.float64)
            assert np.abs(g - fx["guess"][k]).max() < POSE_TOL


@pytest.mark.parametrize("scene", ["640", "720", "640_dist"])
@pytest.mark.parametrize("reproject,pipeline", [(False, True), (True, True), (False, False)])
def test_fused_track_frame_matches_oracle_chain(torch_cuda, oracle, seq640, seq720, seq640_dist, scene, reproject, pipeline):
    """GPU: StreamTracker.step over rendered frames.  CPU: oracle LK + the (reference-validated)
    PoseDetector mirror on the oracle backend, fed per-corner.  Scenes: 640x480, the headline 1280x720 (BASELINE
    configs[1]) and a camera with lens distortion (synthetic.MILD_DIST: frames rendered through it, solvePnP with it)."""
    torch = torch_cuda
    from oracle import cv2_shim
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = {"640": seq640, "720": seq720, "640_dist": seq640_dist}[scene]
    F = len(s)
    # reproject=True rounds the re-projected corners to float32: a 1e-10 pose difference can flip
    # a corner by one float32 ulp (6e-5 px), which LK+PnP turn into ~1e-7 on the next pose.
    tol = 1e-6 if reproject else POSE_TOL
    frames = torch.from_numpy(s.frames()).cuda()                      # [F,H,W]
    trk = StreamTracker(s.width, s.height, s.obj, s.K, s.dist, n_streams=2, reproject=reproject)
    trk.pipeline(pipeline)
    c0 = torch.from_numpy(np.stack([s.corners(0), s.corners(0)])).cuda().contiguous()
    two = lambda k: torch.stack([frames[k], frames[k]]).contiguous()
    f_prev = two(0)
    trk.reset(f_prev, c0)
    so = trk.new_state_buffer()

    import tempfile
    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "april_group.json"), "w").write(json.dumps(s.group))

    class Det(PoseDetector):
        DIRPATH = tmp
    det = Det(LOG, s.K, s.dist, True, cv=cv2_shim.make_cv2())
    obj32 = s.obj.astype(np.float32)
    pts = s.corners(0)
    pyr = oracle.Pyramid(s.frame(0))
    keep = [f_prev]
    for k in range(1, F):
        f = two(k); keep.append(f)
        trk.step(f, so)
        trk.join()
        st = so.cpu().numpy()
        npyr = oracle.Pyramid(s.frame(k))
        nx, status, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, maxLevel=2)
        nx = nx.reshape(-1, 2); status = status.ravel()
        img_list = [nx[i].reshape(1, 1, 2) for i in range(48) if status[i]]
        obj_list = [obj32[i].reshape(1, 3) for i in range(48) if status[i]]
        det._estimate_pose(img_list if len(img_list) >= 8 else [], obj_list if len(img_list) >= 8 else [])
        for b in range(2):
            assert int(st[b, H.ST_NTRACK]) == int(status.sum())
            assert int(st[b, H.ST_OK]) == int(det.last_error is not None and det.last_error < 2)
            ref = np.concatenate([det.last_pose[0].ravel(), det.last_pose[1].ravel()]).astype(np.float64)
            assert np.abs(st[b, :6] - ref).max() < tol, "frame %d" % k
            assert abs(st[b, H.ST_ERR] - det.last_error) < 1e-4          # reference sums float32 norms
            assert np.abs(st[b, :3] - s.rvecs[k]).max() < 3e-3 and np.abs(st[b, 3:6] - s.tvecs[k]).max() < 3e-3
        if reproject and det.last_error is not None and det.last_error < 2:
            pp, _ = oracle.projectPoints(s.obj, det.last_pose[0], det.last_pose[1], s.K, s.dist)
            pts = pp.reshape(-1, 2).astype(np.float32)
        else:
            pts = nx.astype(np.float32)
        pyr = npyr
    states = trk.read_state()
    assert states[0].frame == F - 1 and states[0].has_guess == 1
    g = np.concatenate([det.extrinsic_guess[0].ravel(), det.extrinsic_guess[1].ravel()]).astype(np.float64)
    assert np.abs(np.array(states[1].guess[:]) - g).max() < 10 * tol


@pytest.mark.parametrize("max_level", [2, 3])
def test_pipelined_stream_equals_serial(torch_cuda, seq640, max_level):
    """many frames enqueued back-to-back with NO host sync: the software-pipelined fused step, at every group
    size (frames per launch), must give bit-identical state records to the serial order -- the launch order is
    the only dependency mechanism.  max_level 3 needs a ring of 5 entries per frame of the group."""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    frames = torch.from_numpy(s.frames()).cuda()
    order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 4, 3, 2, 1, 0] * 3
    outs = []
    for depth in (0, 1, 2, 3, 4, 8, 16, 32):
        trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=1, max_level=max_level)
        trk.pipeline(depth)
        trk.reset(frames[0:1].contiguous(), torch.from_numpy(s.corners(0)[None]).cuda().contiguous())
        so = trk.new_state_buffer(len(order))
        for i, k in enumerate(order):
            trk.step(frames[k:k + 1], so[i])
        trk.join()
        outs.append(so.cpu().numpy())
        assert trk.read_state()[0].frame == len(order)
    for o in outs[1:]:
        assert np.array_equal(outs[0], o)
    assert outs[0][:, 0, H.ST_OK].all()


@pytest.mark.parametrize("B,depth", [(1, 1), (1, 5), (1, 20), (3, 4), (44, 2)])
def test_clip_submission_equals_per_frame_calls(torch_cuda, seq640, B, depth):
    """agt_track_frames (StreamTracker.step_many): a clip of K frames in one call is K calls of agt_track_frame -- chained
    fused launches (B = 1, 3; clips shorter, equal to and longer than the launch depth) and the split mode (B = 44)"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    frames = torch.from_numpy(s.frames()).cuda()
    order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0] * 2 + [1, 2, 3]
    clip = torch.stack([frames[k].unsqueeze(0).expand(B, -1, -1) for k in order]).contiguous()       # [23, B, H, W]
    c0 = torch.from_numpy(np.repeat(s.corners(0)[None], B, 0)).cuda().contiguous()
    f0 = frames[0].unsqueeze(0).expand(B, -1, -1).contiguous()
    outs = []
    for cuts in (None, (0, 7, 8, 23), (0, 23)):
        trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=B)
        trk.pipeline(depth)
        trk.reset(f0, c0)
        so = torch.zeros((len(order), B, H.STATE_STRIDE), dtype=torch.float64, device="cuda")
        if cuts is None:
            for i in range(len(order)):
                trk.step(clip[i], so[i])
        else:
            for a, b in zip(cuts[:-1], cuts[1:]):
                trk.step_many(clip[a:b], so[a:b])
        trk.join()
        outs.append(so.cpu().numpy())
        assert trk.read_state()[0].frame == len(order)
    assert outs[0][:, :, H.ST_OK].all() and not (outs[0][:, :, H.ST_FLAGS].astype(int) & H.TRK_CHAIN_TIMEOUT).any()
    for o in outs[1:]:
        assert np.array_equal(outs[0], o)


def test_pipeline_depth_switch_mid_stream(torch_cuda, seq640):
    """changing the group size (or leaving the pipeline) between frames drains the frames in flight and re-seats
    the newest frame's ring entry; the records stay those of the serial order"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    frames = torch.from_numpy(s.frames()).cuda()
    order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 4, 3]
    plan = {0: 4, 7: 1, 11: 0, 14: 8, 20: 2, 23: 3}
    outs = []
    for switching in (False, True):
        trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=2)
        trk.pipeline(0)
        c0 = torch.from_numpy(np.stack([s.corners(0), s.corners(0)])).cuda().contiguous()
        trk.reset(torch.stack([frames[0], frames[0]]).contiguous(), c0)
        so = trk.new_state_buffer(len(order))
        for i, k in enumerate(order):
            if switching and i in plan:
                trk.pipeline(plan[i])
            trk.step(torch.stack([frames[k], frames[k]]).contiguous(), so[i])
        trk.join()
        outs.append(so.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])


def test_track_frame_argument_and_state_errors(torch_cuda):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    obj = np.random.default_rng(0).uniform(-0.05, 0.05, (48, 3))
    trk = StreamTracker(640, 480, obj, np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]), None, n_streams=1)
    f = torch.zeros((1, 480, 640), dtype=torch.uint8, device="cuda")
    with pytest.raises(H.AgtError):
        trk.step(f)                                   # not reset
    trk.reset()
    with pytest.raises(H.AgtError):
        trk.step(f)                                   # reset without corners: only estimate_pose allowed
    # the tag gate wants whole tags: a corner count that is not a multiple of four is refused
    trk46 = StreamTracker(640, 480, obj[:46], np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]]), None, n_streams=1)
    trk46.reset()
    with pytest.raises(H.AgtError):
        trk46.tag_gate(4)
    trk.tag_gate(4); trk.tag_gate(0)
    # fewer than two tags' worth of corners -> guess cleared, no pose
    so = trk.new_state_buffer()
    m = torch.zeros((1, 48), dtype=torch.uint8, device="cuda"); m[0, :4] = 1
    trk.estimate_pose(torch.zeros((1, 48, 2), dtype=torch.float32, device="cuda"), m, so)
    st = so.cpu().numpy()
    assert st[0, H.ST_OK] == 0 and int(st[0, H.ST_FLAGS]) & H.PNP_TOO_FEW and st[0, H.ST_NTRACK] == 4


def test_detector_fed_device_state_machine(tmp_path, oracle):
    """swatbotics-style detections (decision margin filter, missing tags, a frame with
    fewer than two tags) -> dense corner table + mask -> device _estimate_pose, against the PoseDetector
    mirror replaying the same recording on the oracle backend."""
    from oracle import cv2_shim
    from accurate_aprilgroup_tracking_amd import formats, hiplib as HL, synthetic as syn
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    seq = syn.Sequence(640, 480, n_tags=12, n_frames=8, seed=5)
    tag_ids = [int(t) for t in seq.group["tags"].keys()]
    frames = []
    for k in range(8):
        c = seq.corners(k).reshape(-1, 4, 2)
        dets = [formats.make_detection(t, c[i], decision_margin=20.0 if i == (k + 3) % 12 else 75.0)
                for i, t in enumerate(tag_ids) if i != k % 12]
        frames.append(dets[:1] if k == 4 else dets)
    rec = tmp_path / "det.npz"
    formats.save_detections(rec, frames)
    (tmp_path / "april_group.json").write_text(json.dumps(seq.group))
    formats.save_camera_params(tmp_path / "CameraParams.npz", seq.K, np.zeros(5))
    log = logging.getLogger("t"); log.setLevel(logging.CRITICAL)
    det = PoseDetector.from_files(log, tmp_path / "CameraParams.npz", True, cv=cv2_shim.make_cv2(), detector=rec,
                                  april_group=tmp_path / "april_group.json")
    trk = StreamTracker(640, 480, det.all_objpts, seq.K, None, n_streams=1, enhance_ape=True)
    trk.reset()
    out = trk.new_state_buffer()
    replay = formats.ReplayDetector(rec)
    for k in range(8):
        il, ol, ids = det._obtain_detections(None)
        det._estimate_pose(il, ol)
        trk.estimate_pose_from_detections([replay()], tag_ids, out)
        st = out.cpu().numpy()[0]
        if k == 4:
            assert st[HL.ST_OK] == 0
            continue
        assert st[HL.ST_OK] == 1 and st[HL.ST_NTRACK] == 4 * len(ids)
        assert np.abs(st[:3] - det.last_pose[0].ravel()).max() < 1e-8
        assert np.abs(st[3:6] - det.last_pose[1].ravel().astype(np.float64)).max() < 1e-8


def test_stream_1080p_and_240_corners(torch_cuda, oracle, seq1080):
    """BASELINE.json configs[3] (1920x1080 stream, 48 corners, fused step at depth 4) and configs[4]'s corner count
    (60 tags / 240 corners: more than one point per lane, separate-kernel path) against the oracle chain."""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H, synthetic as syn
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    for seq, depth in ((seq1080, 4), (syn.Sequence(1280, 720, n_tags=60, n_frames=4, seed=6, supersample=1), 1)):
        n = seq.obj.shape[0]
        frames = torch.from_numpy(seq.frames()).cuda()
        F = len(seq)
        trk = StreamTracker(seq.width, seq.height, seq.obj, seq.K, None, n_streams=1)
        trk.pipeline(depth)
        trk.reset(frames[0:1].contiguous(), torch.from_numpy(seq.corners(0)[None]).cuda().contiguous())
        so = trk.new_state_buffer(F - 1)
        for k in range(1, F):
            trk.step(frames[k:k + 1], so[k - 1])
        trk.join()
        st = so.cpu().numpy()
        pts = seq.corners(0); pyr = oracle.Pyramid(seq.frame(0))
        r = t = None
        for k in range(1, F):
            npyr = oracle.Pyramid(seq.frame(k))
            nx, status, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, maxLevel=2)
            nx = nx.reshape(-1, 2); ok = status.ravel().astype(bool)
            assert int(st[k - 1, 0, H.ST_NTRACK]) == int(ok.sum()) and ok.sum() >= 8
            dense_model = ok.sum() < n - 8          # 60 tags on the cap overlap in the rendering: most corners are lost, by both
            # first frame: no guess (DLT init); the tracker's later frames start from its motion-model guess, so only
            # the first pose is compared solver-to-solver, the rest against the generator
            if k == 1:
                _, r, t = oracle.solvePnP(seq.obj[ok].astype(np.float32), nx[ok], seq.K, None)
                assert np.abs(st[0, 0, :3] - r.ravel()).max() < 1e-7 and np.abs(st[0, 0, 3:6] - t.ravel()).max() < 1e-7
            if not dense_model:
                assert st[k - 1, 0, H.ST_OK] == 1
                assert np.abs(st[k - 1, 0, :3] - seq.rvecs[k]).max() < 3e-3 and np.abs(st[k - 1, 0, 3:6] - seq.tvecs[k]).max() < 3e-3
            pts = nx.astype(np.float32); pyr = npyr


@pytest.mark.parametrize("win", [13, 27, (17, 11)])
def test_stream_tracker_with_other_lk_windows(torch_cuda, oracle, seq640, win):
    """Round 6 (ABI 504): the stream tracker with an LK window other than 21 x 21 (general LK body, stage-by-stage launches -- the pipelined
    launches exist for the north-star's window only and say so: AGT_ERR_UNSUPPORTED).  Tracked-corner counts equal the oracle chain's,
    the first pose solver to solver, later poses against the generator."""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    seq = seq640
    ww, wh = (win, win) if isinstance(win, int) else win
    code = ww if ww == wh else (ww | (wh << 8))
    frames = torch.from_numpy(seq.frames()).cuda()
    F = min(len(seq), 6)
    trk = StreamTracker(seq.width, seq.height, seq.obj, seq.K, None, n_streams=1, win=code)
    assert trk.ctx.L.agt_tracker_pipeline(trk.ctx.h, 4) == -6          # AGT_ERR_UNSUPPORTED
    trk.pipeline(0)
    trk.reset(frames[0:1].contiguous(), torch.from_numpy(seq.corners(0)[None]).cuda().contiguous())
    so = trk.new_state_buffer(F - 1)
    for k in range(1, F):
        trk.step(frames[k:k + 1], so[k - 1])
    trk.join()
    st = so.cpu().numpy()
    pts = seq.corners(0)
    for k in range(1, F):
        nx, status, _ = oracle.calcOpticalFlowPyrLK(seq.frame(k - 1), seq.frame(k), pts, maxLevel=2, winSize=(ww, wh))
        nx = nx.reshape(-1, 2); ok = status.ravel().astype(bool)
        assert int(st[k - 1, 0, H.ST_NTRACK]) == int(ok.sum()) and ok.sum() >= 8, (k, int(st[k - 1, 0, H.ST_NTRACK]), int(ok.sum()))
        if k == 1:
            _, r, t = oracle.solvePnP(seq.obj[ok].astype(np.float32), nx[ok], seq.K, None)
            assert np.abs(st[0, 0, :3] - r.ravel()).max() < 1e-7 and np.abs(st[0, 0, 3:6] - t.ravel()).max() < 1e-7
        assert st[k - 1, 0, H.ST_OK] == 1
        assert np.abs(st[k - 1, 0, :3] - seq.rvecs[k]).max() < 5e-3 and np.abs(st[k - 1, 0, 3:6] - seq.tvecs[k]).max() < 5e-3
        # (a lost corner stays lost in the tracker: carry the oracle's status the same way)
        pts = nx.astype(np.float32)
        if not ok.all():
            pts = pts.copy(); pts[~ok] = -1e5          # far outside: lost in every later frame, as in the tracker


@pytest.mark.parametrize("camera", ["pinhole", "lens", "tilt"])
def test_240_corners_pipelined_equals_serial(torch_cuda, camera):
    """More than 64 corners per stream: the PnP solve runs on four cooperating waves (agt_pnp_body.h, COOP) -- as the stand-alone
    kernel in serial mode (tracker state in global memory) and as the role of the split pipeline (state in LDS, frames of a group
    in-kernel), with the LK role as a one-frame resp. multi-frame group launch.  A 60-tag scene that keeps all 240 corners:
    the records of every depth are bitwise those of the serial order, all frames accepted from a guess after the first.
    camera (round 5): also through a distorting lens (frames rendered through it) and through a tilted camera model (solver-side only) --
    the group kernel's distortion branch, compiled without MachineLICM in its own translation unit, against the stand-alone kernel's."""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H, synthetic as syn
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = syn.Sequence(1280, 720, n_tags=60, n_frames=7, seed=8, supersample=2, dist=syn.MILD_DIST if camera == "lens" else None)
    dist = s.dist if camera != "tilt" else np.array([[0.01, -0.005, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.003, -0.002]])
    assert s.obj.shape[0] == 240
    frames = torch.from_numpy(s.frames()).cuda()
    order = [1, 2, 3, 4, 5, 6, 5, 4, 3, 2, 1, 0, 1, 2]
    outs = {}
    for depth in (0, 1, 3, 8):
        trk = StreamTracker(s.width, s.height, s.obj, s.K, dist, n_streams=1)
        trk.pipeline(depth)
        trk.reset(frames[0:1].contiguous(), torch.from_numpy(s.corners(0)[None]).cuda().contiguous())
        so = trk.new_state_buffer(len(order))
        for i, k in enumerate(order):
            trk.step(frames[k:k + 1], so[i])
        trk.join()
        torch.cuda.synchronize()
        outs[depth] = so.cpu().numpy()[:, 0]
    ref = outs[0]
    assert ref[:, H.ST_OK].all() and (ref[:, H.ST_NTRACK] == 240).all() and ref[1:, H.ST_GUESS].all() and ref[0, H.ST_GUESS] == 0
    for k, i in enumerate(order):
        assert camera == "tilt" or (np.abs(ref[k, :3] - s.rvecs[i]).max() < 3e-3 and np.abs(ref[k, 3:6] - s.tvecs[i]).max() < 3e-3)
    for depth in (1, 3, 8):
        assert np.array_equal(outs[depth].view(np.uint64), ref.view(np.uint64)), "depth %d differs from the serial order" % depth


def test_group_with_changing_frame_pitch(torch_cuda, seq640):
    """frames of one launch group must share pitch and batch stride; a stream that alternates between tight and padded
    frame buffers makes the library cut its groups short -- the records stay those of the serial order"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    frames = torch.from_numpy(s.frames()).cuda()
    H, W = s.height, s.width
    order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2, 3]
    padded = torch.zeros((len(order), 1, H, W + 64), dtype=torch.uint8, device="cuda")
    outs = []
    for depth in (0, 1, 2, 4, 16):
        trk = StreamTracker(W, H, s.obj, s.K, None, n_streams=1)
        trk.pipeline(depth)
        trk.reset(frames[0:1].contiguous(), torch.from_numpy(s.corners(0)[None]).cuda().contiguous())
        so = trk.new_state_buffer(len(order))
        for i, k in enumerate(order):
            if i % 3 == 1 or i in (10, 11, 12, 13, 14):
                padded[i, 0, :, :W] = frames[k]
                f = padded[i, :, :, :W]                     # pitch W + 64
            else:
                f = frames[k:k + 1]
            trk.step(f, so[i])
        trk.join()
        outs.append(so.cpu().numpy())
    for o in outs[1:]:
        assert np.array_equal(outs[0], o)
    assert outs[0][:, 0, 6].all()


def test_batch64_720p_is_batch_invariant(torch_cuda, seq720):
    """BASELINE.json configs[2] size (64 x 1280x720 per step): every stream of a 64-stream batch (stage kernels on
    three overlapped streams, one wave per corner, ring-reuse guards every 4th frame) must produce bit-for-bit the
    record a single stream gets from the fused step (four waves per corner, PnP role in the launch) -- the results may
    not depend on batching, kernel variant or pipelining."""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq720
    frames = torch.from_numpy(s.frames()).cuda()
    F = len(s)
    order = (list(range(1, F)) + list(range(F - 2, -1, -1))) * 6 + list(range(1, F))      # 39 steps, never synchronised
    recs = {}
    # (40 streams x 48 corners = 1920: the fused launch with one wave per corner in the LK role, two workgroups per CU, 40
    # PnP workgroups of two alternating waves chained to it; 64: split mode with the LK launches on two streams)
    for B, depth in ((1, 4), (64, 1), (8, 2), (40, 8), (64, 16)):
        trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=B)
        trk.pipeline(depth)
        rep = lambda k: frames[k].unsqueeze(0).expand(B, -1, -1).contiguous()
        trk.reset(rep(0), torch.from_numpy(np.repeat(s.corners(0)[None], B, 0)).cuda().contiguous())
        so = trk.new_state_buffer(len(order))
        keep = []
        for i, k in enumerate(order):
            f = rep(k); keep.append(f)
            trk.step(f, so[i] if len(order) > 1 else so)
        trk.join()
        recs[(B, depth)] = so.cpu().numpy().reshape(len(order), B, -1)
        if B == 64:
            # a reset while frames are still in flight on the library's streams (no join, no sync) starts a clean run
            for i, k in enumerate(order[:7]):
                f = rep(k); keep.append(f)
                trk.step(f, so[i])
            trk.reset(rep(0), torch.from_numpy(np.repeat(s.corners(0)[None], B, 0)).cuda().contiguous())
            so2 = trk.new_state_buffer(6)
            for i, k in enumerate(order[:6]):
                f = rep(k); keep.append(f)
                trk.step(f, so2[i])
            trk.join()
            assert np.array_equal(so2.cpu().numpy().reshape(6, B, -1), recs[(64, depth)][:6])
    for (B, depth), r in recs.items():
        for b in range(B):
            assert np.array_equal(r[:, b], recs[(1, 4)][:, 0]), "stream %d of %d at depth %d" % (b, B, depth)
    assert recs[(1, 4)][:, 0, 6].all()


def test_split_pipeline_blocks_repeat_bitwise(torch_cuda, seq720):
    """Round 6 (the short form of tools/soak.py, which ran 46,621 such blocks: profiles/r06_soak.txt): the 64-stream split pipeline is
    deterministic -- 60 blocks of the same 39 steps from the same reset state give bitwise the same records, every stream the same as
    stream 0, none flagged.  A table entry read before it was written, a stale pointer or a lost state update (the class of defect behind
    round 5's aperture violation, which ALSO produced silently wrong poses once per ~1,000 launches) shows here as a differing block."""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq720
    B = 64
    F = len(s)
    frames = torch.from_numpy(s.frames()).cuda()
    reps = [frames[k].unsqueeze(0).expand(B, -1, -1).contiguous() for k in range(F)]
    order = (list(range(1, F)) + list(range(F - 2, -1, -1))) * 3 + list(range(1, F))
    c0 = torch.from_numpy(np.repeat(s.corners(0)[None], B, 0)).cuda().contiguous()
    trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=B)
    trk.pipeline(16)
    so = trk.new_state_buffer(len(order))
    ref = None
    for blk in range(60):
        so.zero_()
        trk.reset(reps[0], c0)
        for i, k in enumerate(order):
            trk.step(reps[k], so[i])
        trk.join()
        assert trk.ctx.L.agt_synchronize(trk.ctx.h) == 0
        r = so.cpu().numpy().view(np.uint64)
        if ref is None:
            ref = r.copy()
            rec = so.cpu().numpy()
            assert rec[:, :, H.ST_OK].all() and not ((rec[:, :, 11].astype(np.int64) & 512) != 0).any()
            assert all(np.array_equal(ref[:, b], ref[:, 0]) for b in range(B))
        else:
            assert np.array_equal(r, ref), "block %d differs from block 0 in %d words" % (blk, int((r != ref).sum()))


def test_mode_changes_between_runs(torch_cuda, seq640):
    """one context, several runs: 44-stream batch on the library's streams at depth 4, then (reset) a single stream on
    the fused step at depth 4, then the batch again -- ring sizes and moduli follow; every run equals a fresh tracker"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    frames = torch.from_numpy(s.frames()).cuda()
    order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 4, 3, 2, 1]

    def run(trk, B):
        rep = lambda k: frames[k].unsqueeze(0).expand(B, -1, -1).contiguous()
        trk.reset(rep(0), torch.from_numpy(np.repeat(s.corners(0)[None], B, 0)).cuda().contiguous())
        so = torch.zeros((len(order), B, 16), dtype=torch.float64, device="cuda")
        keep = []
        for i, k in enumerate(order):
            f = rep(k); keep.append(f)
            trk.step(f, so[i])
        trk.join()
        return so.cpu().numpy()

    ref = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=1)
    ref.pipeline(0)
    want = run(ref, 1)[:, 0]
    trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=44)     # 2112 corners: past the fused cut-off
    trk.pipeline(4)
    for B in (44, 1, 44, 3):
        trk.B = B
        got = run(trk, B)
        for b in range(B):
            assert np.array_equal(got[:, b], want), "B=%d stream %d" % (B, b)


@pytest.mark.parametrize("B,depth", [(64, 1), (1, 4), (2, 1)])
def test_reset_mid_flight_at_every_ring_phase(torch_cuda, seq640, B, depth):
    """StreamTracker.reset builds its frame into ring entry 0 -- with frames still in flight (library
    streams at B = 64, unlaunched groups of the fused pipeline otherwise) that build must be ordered behind them, at
    every phase of the ring (a reset after 5..12 un-joined frames covers the newest frame sitting in entry 0)."""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    frames = torch.from_numpy(s.frames()).cuda()
    rep = lambda k: frames[k].unsqueeze(0).expand(B, -1, -1).contiguous()
    c0 = torch.from_numpy(np.repeat(s.corners(0)[None], B, 0)).cuda().contiguous()
    order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5]
    trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=B)
    trk.pipeline(depth)
    want = None
    keep = []
    for pre in (0, 5, 6, 7, 8, 9, 10, 11, 12):
        if pre:
            trk.reset(rep(0), c0)
            for k in order[:pre]:
                f = rep(k); keep.append(f)
                trk.step(f, None)                      # left in flight: no join, no sync
        trk.reset(rep(0), c0)
        so = trk.new_state_buffer(6)
        for i, k in enumerate(order[:6]):
            f = rep(k); keep.append(f)
            trk.step(f, so[i])
        trk.join()
        got = so.cpu().numpy().reshape(6, B, -1)
        if want is None:
            want = got
            assert want[:, 0, 6].all()
        assert np.array_equal(got, want), "reset after %d frames in flight" % pre


def test_lost_corner_stays_lost(torch_cuda, oracle, seq640):
    """LK status is sticky in the tracker.  Two corners are pushed out of the image for one frame (their
    positions are overwritten in the live corner buffer); afterwards the texture under their last position would let
    LK 'track' again -- the tracker must keep them masked (status 0, position carried) in every later frame, in every
    launch mode, and the pose must equal the oracle chain with the same rule."""
    torch = torch_cuda
    import ctypes as C
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    frames = torch.from_numpy(s.frames()).cuda()
    F = len(s)
    c0 = s.corners(0).copy()
    lost = [5, 17]
    c0[lost[0]] = (-40.0, 100.0)           # window wholly outside: status 0 at level 0
    c0[lost[1]] = (s.width + 35.0, 50.0)
    # oracle chain with the sticky rule
    pts = c0.copy(); alive = np.ones(48, bool); pyr = oracle.Pyramid(s.frame(0))
    ref_status, ref_pts = [], []
    for k in range(1, F):
        npyr = oracle.Pyramid(s.frame(k))
        nx, st, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, maxLevel=2)
        nx = nx.reshape(-1, 2); st = st.ravel().astype(bool)
        nx[~alive] = pts[~alive]
        alive &= st
        ref_status.append(alive.copy()); ref_pts.append(nx.copy())
        pts = nx.astype(np.float32); pyr = npyr
    assert not ref_status[0][lost].any()
    outs = []
    for depth in (0, 1, 4):
        trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=1)
        trk.pipeline(depth)
        trk.reset(frames[0:1].contiguous(), torch.from_numpy(c0[None]).cuda().contiguous())
        so = trk.new_state_buffer(F - 1)
        for k in range(1, F):
            trk.step(frames[k:k + 1], so[k - 1])
        trk.join()
        st = so.cpu().numpy()
        outs.append(st)
        for k in range(1, F):
            assert int(st[k - 1, 0, H.ST_NTRACK]) == int(ref_status[k - 1].sum())
        cp, sp = trk.corners()
        torch.cuda.synchronize()
        got_c = np.zeros((48, 2), np.float32); got_s = np.zeros(48, np.uint8)
        H.check(trk.ctx.L.agt_download(trk.ctx.h, got_c.ctypes.data_as(C.c_void_p), C.c_void_p(cp), got_c.nbytes), "agt_download")
        H.check(trk.ctx.L.agt_download(trk.ctx.h, got_s.ctypes.data_as(C.c_void_p), C.c_void_p(sp), got_s.nbytes), "agt_download")
        assert np.array_equal(got_s.astype(bool), ref_status[-1])
        assert np.array_equal(got_c.view(np.uint32), ref_pts[-1].astype(np.float32).view(np.uint32))
        ok = ref_status[-1]
        _, r, t = oracle.solvePnP(s.obj[ok].astype(np.float32), ref_pts[-1][ok].astype(np.float32), s.K, None,
                                  s.rvecs[F - 1], s.tvecs[F - 1], True)
        assert np.abs(st[-1, 0, :3] - r.ravel()).max() < 1e-6 and np.abs(st[-1, 0, 3:6] - t.ravel()).max() < 1e-6
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


def test_chained_lk_role_big_motion_and_image_border(torch_cuda, oracle, seq640):
    """The frame-chained LK role of the fused step (agt_lk_chain_body.h) on what its fast path does not cover: frames taken
    out of order (jumps of up to five frames: flows past the 9 px tile margin -> search tiles re-staged, previous-image
    tiles reloaded) on a crop that leaves corners a few pixels from the left / top image border (windows and tiles reach
    outside: reflected tile loads, no prefetch for those levels).  Corners and status after every launch mode equal the
    oracle's LK chain bit for bit; records equal the stage-by-stage mode."""
    torch = torch_cuda
    import ctypes as C
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    all_c = np.stack([s.corners(k) for k in range(len(s))])
    x0 = int(max(0, np.floor(all_c[..., 0].min()) - 6)) & ~3
    y0 = int(max(0, np.floor(all_c[..., 1].min()) - 4))
    fr = s.frames()[:, y0:, x0:]
    Hc, Wc = fr.shape[1], fr.shape[2] & ~3
    fr = np.ascontiguousarray(fr[:, :, :Wc])
    # two more "frames": frames 2 and 4 displaced by (+11, -7) px as a whole (wrap-around at the far borders), so that a
    # step onto / off them is a flow beyond the tile margin at level 0
    fr = np.concatenate([fr, np.roll(fr[2:3], (-7, 11), axis=(1, 2)), np.roll(fr[4:5], (-7, 11), axis=(1, 2))])
    Kc = s.K.copy(); Kc[0, 2] -= x0; Kc[1, 2] -= y0
    shift = np.array([x0, y0], np.float32)
    order = [3, 0, 6, 1, 7, 4, 0, 5, 6, 2, 3]
    c0 = (s.corners(0) - shift).astype(np.float32)
    assert c0[:, 0].min() < 10.5 or c0[:, 1].min() < 10.5        # some window starts outside the image
    # oracle LK chain with the tracker's sticky status
    pts = c0.copy(); alive = np.ones(len(c0), bool); pyr = oracle.Pyramid(fr[0])
    big = 0.0
    for k in order:
        npyr = oracle.Pyramid(fr[k])
        nx, st, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, maxLevel=2)
        nx = nx.reshape(-1, 2); st = st.ravel().astype(bool)
        nx[~alive] = pts[~alive]
        big = max(big, float(np.abs(nx[alive & st] - pts[alive & st]).max()) if (alive & st).any() else 0.0)
        alive &= st
        pts = nx.astype(np.float32); pyr = npyr
    assert big > 9.0 and alive.sum() >= 8
    frames = torch.from_numpy(fr).cuda()
    outs = []
    for depth in (0, 1, 4, 16):
        trk = StreamTracker(Wc, Hc, s.obj, Kc, None, n_streams=1)
        trk.pipeline(depth)
        trk.reset(frames[0:1].contiguous(), torch.from_numpy(c0[None]).cuda().contiguous())
        so = trk.new_state_buffer(len(order))
        for i, k in enumerate(order):
            trk.step(frames[k:k + 1], so[i])
        trk.join()
        outs.append(so.cpu().numpy())
        cp, sp = trk.corners()
        torch.cuda.synchronize()
        got_c = np.zeros((len(c0), 2), np.float32); got_s = np.zeros(len(c0), np.uint8)
        H.check(trk.ctx.L.agt_download(trk.ctx.h, got_c.ctypes.data_as(C.c_void_p), C.c_void_p(cp), got_c.nbytes), "agt_download")
        H.check(trk.ctx.L.agt_download(trk.ctx.h, got_s.ctypes.data_as(C.c_void_p), C.c_void_p(sp), got_s.nbytes), "agt_download")
        assert np.array_equal(got_s.astype(bool), alive), "depth %d" % depth
        assert np.array_equal(got_c.view(np.uint32), pts.view(np.uint32)), "depth %d" % depth
        assert not (outs[-1][:, :, H.ST_FLAGS].astype(int) & H.TRK_CHAIN_TIMEOUT).any()
    for o in outs[1:]:
        assert np.array_equal(outs[0], o)


_GIVE_UP_CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, os.environ["AGT_REPO_ROOT"])
from accurate_aprilgroup_tracking_amd import hiplib as H
H.LIB_PATH = os.path.join(os.environ["AGT_REPO_ROOT"], "accurate_aprilgroup_tracking_amd", "libagt_hip_dbg.so")
import torch
from accurate_aprilgroup_tracking_amd import synthetic as syn
from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
s = syn.Sequence(640, 480, n_tags=12, n_frames=6, seed=0)
frames = torch.from_numpy(s.frames()).cuda()
order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2]
c0 = torch.from_numpy(s.corners(0)[None]).cuda().contiguous()
trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=1)
trk.pipeline(4)
out = {}
def run(tag):
    trk.reset(frames[0:1].contiguous(), c0)
    so = trk.new_state_buffer(len(order))
    codes = []
    for i, k in enumerate(order):
        trk.step(frames[k:k + 1], so[i])
    try:
        trk.join(); codes.append(0)
    except H.AgtError as e:
        codes.append(e.code)
    codes.append(trk.ctx.L.agt_synchronize(trk.ctx.h))
    st = trk.read_state()[0]
    out[tag] = dict(rec=so.cpu().numpy()[:, 0].tolist(), codes=codes, chain_fault=st.chain_fault, frame=st.frame,
                    prev=list(st.prev[:]), has_prev=st.has_prev)
run("faulted")          # AGT_CHAIN_WITHHOLD=2: the second launch with chained waits never sees its second waited frame complete
run("recovered")        # the knob has fired; agt_tracker_reset must bring the stream back
print("RESULT " + json.dumps(out))
'''


def test_chain_give_up_is_fail_stop(torch_cuda, seq640):
    """VERDICT r2 #8 / ADVICE r2 (medium): the give-up path of the chained launch, executed once.  The diagnostic library
    (make dbg: AGT_DEBUG_KNOBS) withholds one arrival from the PnP role of one launch (AGT_CHAIN_WITHHOLD).  Expected:
    the waiting wave gives up after its poll budget, does NOT solve on the stale ring entry, flags the record
    AGT_TRK_CHAIN_TIMEOUT and zeroes it; the stream's tracker state stays that of the last good frame; every later record of
    the stream is flagged too and nothing waits again (the launch drains, the run ends); agt_synchronize returns
    AGT_ERR_CHAIN; agt_tracker_reset recovers and the records of a clean run come back bit for bit."""
    import subprocess
    import sys
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dbg = os.path.join(root, "accurate_aprilgroup_tracking_amd", "libagt_hip_dbg.so")
    if not os.path.exists(dbg):
        subprocess.check_call(["make", "-s", "-j", "8", "-C", os.path.join(root, "accurate_aprilgroup_tracking_amd", "csrc"), "dbg"])
    env = dict(os.environ, AGT_CHAIN_WITHHOLD="2", AGT_REPO_ROOT=root)
    res = subprocess.run([sys.executable, "-c", _GIVE_UP_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    # the undisturbed run, on the product library in this process
    s = seq640
    frames = torch.from_numpy(s.frames()).cuda()
    order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2]
    trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=1)
    trk.pipeline(4)
    trk.reset(frames[0:1].contiguous(), torch.from_numpy(s.corners(0)[None]).cuda().contiguous())
    so = trk.new_state_buffer(len(order))
    for i, k in enumerate(order):
        trk.step(frames[k:k + 1], so[i])
    trk.join()
    clean = so.cpu().numpy()[:, 0]
    assert clean[:, H.ST_OK].all()
    f = out["faulted"]
    rec = np.array(f["rec"])
    flags = rec[:, H.ST_FLAGS].astype(int)
    bad = np.nonzero(flags & H.TRK_CHAIN_TIMEOUT)[0]
    assert len(bad) and bad[0] >= 4, "the withheld arrival belongs to the second chained launch"
    first = int(bad[0])
    assert np.array_equal(bad, np.arange(first, len(order))), "every record after the give-up is flagged (sticky fault)"
    assert np.array_equal(rec[:first], clean[:first]), "records before the give-up are those of the clean run, bit for bit"
    assert (rec[first:, :8] == 0).all(), "nothing is solved on a stale ring entry: invalid records are zero"
    assert f["chain_fault"] == 1 and f["frame"] == len(order)
    assert f["has_prev"] == 1 and np.array_equal(np.array(f["prev"]), clean[first - 1, :6]), "tracker state frozen at the last good frame"
    assert f["codes"][1] == -8, "agt_synchronize reports AGT_ERR_CHAIN"
    r = out["recovered"]
    assert r["codes"] == [0, 0] and r["chain_fault"] == 0
    assert np.array_equal(np.array(r["rec"]), clean), "agt_tracker_reset recovers the stream"


_POISON_CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, os.environ["AGT_REPO_ROOT"])
from accurate_aprilgroup_tracking_amd import hiplib as H
H.LIB_PATH = os.path.join(os.environ["AGT_REPO_ROOT"], "accurate_aprilgroup_tracking_amd", "libagt_hip_dbg.so")
import torch
from accurate_aprilgroup_tracking_amd import synthetic as syn
from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
B = int(os.environ["AGT_TEST_STREAMS"])
s = syn.Sequence(640, 480, n_tags=12, n_frames=6, seed=0)
frames = torch.from_numpy(s.frames()).cuda()
order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2]
c0 = torch.from_numpy(np.repeat(s.corners(0)[None], B, 0)).cuda().contiguous()
trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=B)
trk.pipeline(4)
out = {}
def run(tag):
    trk.reset(frames[0:1].repeat(B, 1, 1).contiguous(), c0)
    so = trk.new_state_buffer(len(order))
    codes = []
    keep = []
    for i, k in enumerate(order):
        f = frames[k:k + 1].repeat(B, 1, 1).contiguous(); keep.append(f)
        trk.step(f, so[i])
    try:
        trk.join(); codes.append(0)
    except H.AgtError as e:
        codes.append(e.code)
    codes.append(trk.ctx.L.agt_synchronize(trk.ctx.h))
    st = trk.read_state()
    out[tag] = dict(rec=so.cpu().numpy().tolist(), codes=codes, chain_fault=[x.chain_fault for x in st])
run("faulted")          # the knob poisons one table entry of one launch
run("recovered")        # the knob has fired; agt_tracker_reset must bring the streams back
print("RESULT " + json.dumps(out))
'''


@pytest.mark.parametrize("role,streams", [("PNP", 1), ("LK", 1), ("PNP", 8), ("LK", 8)])
def test_poisoned_table_entry_is_fail_stop(torch_cuda, seq640, role, streams):
    """a per-frame table entry that cannot be an address -- what a stale or clobbered LDS copy of the
    kernel-argument tables would hand a role -- is never dereferenced.  The diagnostic library puts the bits of a NaN into the
    second frame's entry of one launch (AGT_TABLE_POISON_PNP / _LK); one stream runs the fused chained step (step_kernel), eight
    streams the split pipeline (pnp_group_kernel<1> / lk_group_kernel).  Expected: no GPU fault (the child exits 0, the queue is
    not aborted with HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION), the launch drains, agt_synchronize reports AGT_ERR_CHAIN, frames
    before the poisoned one are those of a clean run, and agt_tracker_reset brings the streams back bit for bit."""
    import subprocess
    import sys
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dbg = os.path.join(root, "accurate_aprilgroup_tracking_amd", "libagt_hip_dbg.so")
    if not os.path.exists(dbg):
        subprocess.check_call(["make", "-s", "-j", "8", "-C", os.path.join(root, "accurate_aprilgroup_tracking_amd", "csrc"), "dbg"])
    env = dict(os.environ, AGT_REPO_ROOT=root, AGT_TEST_STREAMS=str(streams))
    env["AGT_TABLE_POISON_" + role] = "2"
    res = subprocess.run([sys.executable, "-c", _POISON_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    s = seq640
    frames = torch.from_numpy(s.frames()).cuda()
    order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2]
    B = streams
    trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=B)
    trk.pipeline(4)
    trk.reset(frames[0:1].repeat(B, 1, 1).contiguous(), torch.from_numpy(np.repeat(s.corners(0)[None], B, 0)).cuda().contiguous())
    so = trk.new_state_buffer(len(order))
    keep = []
    for i, k in enumerate(order):
        keep.append(frames[k:k + 1].repeat(B, 1, 1).contiguous())
        trk.step(keep[-1], so[i])
    trk.join()
    clean = so.cpu().numpy()
    assert clean[:, :, H.ST_OK].all()
    f, r = out["faulted"], out["recovered"]
    rec = np.array(f["rec"])
    assert f["codes"][1] == -8, "agt_synchronize reports AGT_ERR_CHAIN (codes %s)" % f["codes"]
    differs = np.nonzero((rec != clean).any(axis=(1, 2)))[0]
    # (the fused step runs groups of four frames from the start; the split pipeline fills in groups of two, then four: agt_tracker_frames.hip split_ramp)
    first_ok = 4 if streams == 1 else 2
    assert len(differs) and differs[0] >= first_ok, "the poisoned entry belongs to the second multi-frame launch: the frames of the first one are clean"
    if role == "PNP" or streams == 1:
        # the pose role saw the poisoned entry itself (PNP) or gave up waiting for the LK role that did (LK, chained): flagged records
        flags = rec[:, :, H.ST_FLAGS].astype(int)
        assert (flags[differs[0]:] & H.TRK_CHAIN_TIMEOUT).all() and not (flags[:differs[0]] & H.TRK_CHAIN_TIMEOUT).any()
        assert (rec[differs[0]:, :, :8] == 0).all(), "nothing is solved behind a table entry that is not an address"
        assert all(f["chain_fault"])
    assert r["codes"] == [0, 0] and not any(r["chain_fault"])
    assert np.array_equal(np.array(r["rec"]), clean), "agt_tracker_reset recovers the streams"


def test_context_lifetime_returns_memory_and_keeps_the_split_pipeline_fast(torch_cuda, seq640):
    """200 x agt_create -> a tracked clip on the split pipeline (eight streams: pyramid / LK / pose launches on the caller's
    stream and three library streams, events between them) -> agt_destroy.  Device memory comes back (no more than 1 MiB less free than at
    the start), every context's records are those of the first, and a context created after the 200 still runs the split pipeline at the
    first one's speed: the library's streams are a process-wide pool (agt_api.hip ms_pool_acquire) -- streams created and destroyed per
    context left later ones sharing hardware queues, 1.5-1.8 x slower."""
    import time
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    B = 8
    frames = [torch.from_numpy(s.frame(k)).cuda().unsqueeze(0).repeat(B, 1, 1).contiguous() for k in range(6)]
    c0 = torch.from_numpy(np.repeat(s.corners(0)[None], B, 0)).cuda().contiguous()
    order = [1, 2, 3, 4, 5, 4, 3, 2]
    so = torch.zeros((len(order), B, 16), dtype=torch.float64, device="cuda")

    def run(trk, reps=1):
        t = None
        for _ in range(reps):
            trk.reset(frames[0], c0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i, k in enumerate(order):
                trk.step(frames[k], so[i])
            trk.join()
            torch.cuda.synchronize()
            t = time.perf_counter() - t0
        return t, so.cpu().numpy().copy()

    def make():
        trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=B)
        trk.pipeline(4)
        return trk

    first = make()
    t_first = min(run(first, 3)[0] for _ in range(3))
    ref = run(first)[1]
    assert ref[:, :, 6].all(), "every frame of every stream accepted"
    first.ctx.close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(200):
        trk = make()
        _, rec = run(trk)
        assert np.array_equal(rec, ref), "context %d" % i
        trk.ctx.close()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    # (one-sided: the runtime may hand memory back late -- the first context's 48 MiB showed up as FREE only after the loop -- a leak shows as less)
    assert free0 - free1 <= (1 << 20), "device memory after 200 contexts: %d B free against %d B before them" % (free1, free0)
    last = make()
    t_last = min(run(last, 3)[0] for _ in range(3))
    assert np.array_equal(run(last)[1], ref)
    last.ctx.close()
    assert t_last <= 1.3 * t_first, "split pipeline after 200 contexts: %.1f us against %.1f us for the first" % (t_last * 1e6, t_first * 1e6)
