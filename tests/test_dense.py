"""Dense photometric pose refinement (BASELINE configs[4] / SURVEY a12, 8f rank 2).  No reference code
exists; the specification lives in oracle/cv_dense.c.  CPU: the oracle satisfies its own spec
(finite-difference Jacobian, convergence to a known pose).  GPU: HIP vs oracle."""
import ctypes as C
import os
import numpy as np
import pytest

from accurate_aprilgroup_tracking_amd import synthetic as syn


@pytest.fixture(scope="module")
def scene():
    s = syn.Sequence(1280, 720, n_tags=12, n_frames=3, seed=5, supersample=3)
    mx = syn.model_samples(s.group, 32)
    return s, mx


def _template(s, mx, k):
    return np.nan_to_num(syn.sample_bilinear(s.frame(k), syn.project(mx, s.rvecs[k], s.tvecs[k], s.K)), nan=128.0).astype(np.float32)


def test_photometric_rows_follow_the_specification(oracle, scene):
    """r_i and dr_i/dp against an independent numpy statement of the spec (bilinear intensity,
    bilinearly interpolated central-difference gradient), and the cost gradient J^T r against finite
    differences of the cost (the interpolated gradient is a smoothed derivative, so directions --
    not individual entries -- are compared)."""
    s, mx = scene
    f = s.frame(1).astype(np.float64)
    L = oracle.lib()
    L.cvo_dense_sample.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p,
                                   C.c_double, C.c_void_p, C.c_void_p]
    f8 = s.frame(1)
    gxi = np.zeros_like(f); gyi = np.zeros_like(f)
    gxi[:, 1:-1] = (f[:, 2:] - f[:, :-2]) * 0.5
    gyi[1:-1, :] = (f[2:, :] - f[:-2, :]) * 0.5
    T = 100.0

    def rows(pp, idx, use_oracle):
        nonlocal f8
        uv, jac = oracle.projectPoints(mx[idx].astype(np.float64), pp[:3], pp[3:], s.K, None, jacobian=True)
        uv = uv.reshape(-1, 2)
        if not use_oracle:
            I = syn.sample_bilinear(f, uv); gx = syn.sample_bilinear(gxi, uv); gy = syn.sample_bilinear(gyi, uv)
            return I - T, gx[:, None] * jac[0::2] + gy[:, None] * jac[1::2]
        out_r, out_j = [], []
        for n in range(len(idx)):
            ju = np.ascontiguousarray(jac[2 * n]); jv = np.ascontiguousarray(jac[2 * n + 1])
            r = C.c_double(); J = np.zeros(6)
            assert L.cvo_dense_sample(f8.ctypes.data, 1280, 720, f8.strides[0], float(uv[n, 0]), float(uv[n, 1]),
                                      ju.ctypes.data, jv.ctypes.data, T, C.byref(r), J.ctypes.data)
            out_r.append(r.value); out_j.append(J)
        return np.array(out_r), np.array(out_j)
    p = np.concatenate([s.rvecs[1], s.tvecs[1]])
    idx = np.arange(0, len(mx), 97)
    uv0 = syn.project(mx[idx], s.rvecs[1], s.tvecs[1], s.K)
    inside = (uv0[:, 0] > 4) & (uv0[:, 0] < 1280 - 6) & (uv0[:, 1] > 4) & (uv0[:, 1] < 720 - 6)     # valid for every perturbed pose below
    idx = idx[inside]
    assert len(idx) > 100
    r_o, J_o = rows(p, idx, True)
    r_n, J_n = rows(p, idx, False)
    assert np.abs(r_o - r_n).max() < 1e-9 and np.abs(J_o - J_n).max() < 1e-7 * np.abs(J_n).max()
    # samples whose 2x2 cell touches the frame border are invalid
    r = C.c_double(); J = np.zeros(6); z = np.zeros(6)
    for (u, v, ok) in ((0.5, 100.0, 0), (1.0, 1.0, 1), (1277.99, 300.0, 1), (1278.0, 300.0, 0), (640.0, 717.99, 1), (640.0, 718.0, 0), (-3.0, 5.0, 0)):
        assert L.cvo_dense_sample(f8.ctypes.data, 1280, 720, f8.strides[0], u, v, z.ctypes.data, z.ctypes.data, 0.0, C.byref(r), J.ctypes.data) == ok
    # cost gradient direction on a band-limited version of the frame (where central differences are a
    # faithful derivative): J^T r must point along the finite-difference gradient of the cost
    from scipy.ndimage import gaussian_filter
    f8 = np.clip(np.rint(gaussian_filter(f, 2.5)), 0, 255).astype(np.uint8)
    r_o, J_o = rows(p, idx, True)
    g = J_o.T @ r_o
    num = np.zeros(6)
    for k in range(6):
        d = np.zeros(6); d[k] = 1e-4 if k < 3 else 1e-5
        num[k] = (0.5 * (rows(p + d, idx, True)[0] ** 2).sum() - 0.5 * (rows(p - d, idx, True)[0] ** 2).sum()) / (2 * d[k])
    scale = np.array([1, 1, 1, 10, 10, 10.0])       # rvec / tvec entries live on different scales
    cosang = (g / scale) @ (num / scale) / (np.linalg.norm(g / scale) * np.linalg.norm(num / scale))
    assert cosang > 0.97


def test_oracle_converges_to_known_pose(oracle, scene):
    s, mx = scene
    f = s.frame(1)
    T = _template(s, mx, 1)
    r0 = s.rvecs[1] + np.array([0.004, -0.003, 0.002]); t0 = s.tvecs[1] + np.array([0.0004, -0.0003, 0.001])
    assert np.abs(syn.project(s.obj, r0, t0, s.K) - s.corners(1)).max() > 2.0            # starts > 2 px off
    r, t, st = oracle.dense_refine(f, mx, T, None, None, None, s.K, None, r0, t0, iters=10, photo_weight=1.0)
    assert st["valid"] > 0.95 * len(mx) and st["photo_rms"] < 0.05
    assert np.abs(r - s.rvecs[1]).max() < 1e-6 and np.abs(t - s.tvecs[1]).max() < 1e-6
    # template from the previous frame, joint with the corner term: lands near the true pose of frame 1
    T0 = _template(s, mx, 0)
    r, t, st = oracle.dense_refine(f, mx, T0, s.obj, s.corners(1), None, s.K, None, s.rvecs[0], s.tvecs[0], iters=10, photo_weight=0.01)
    assert np.abs(r - s.rvecs[1]).max() < 5e-4 and np.abs(t - s.tvecs[1]).max() < 5e-5 and st["used"] == 48
    # early stop fires
    r2, t2, st2 = oracle.dense_refine(f, mx, T, None, None, None, s.K, None, s.rvecs[1], s.tvecs[1], iters=50, photo_weight=1.0)
    assert st2["iters"] < 50


# (round 5: "tilt" = the 14-coefficient model with a tilted sensor -- the dense stage projects through agt_project like the solver)
TILT14 = np.array([[0.02, -0.01, 1e-3, -1e-3, 0.005, 0.01, -0.005, 0.002, 5e-4, -5e-4, 2e-4, 3e-4, 0.004, -0.003]])


@pytest.mark.gpu
@pytest.mark.parametrize("use_dist", [False, True, "tilt"])
def test_hip_matches_oracle(oracle, scene, use_dist):
    import torch
    from accurate_aprilgroup_tracking_amd import cv_hip
    s, mx = scene
    dist = TILT14 if use_dist == "tilt" else (syn.MILD_DIST if use_dist else None)
    T = _template(s, mx, 1)
    rng = np.random.default_rng(1)
    B = 3
    starts = [np.concatenate([s.rvecs[1] + rng.normal(0, 0.003, 3), s.tvecs[1] + rng.normal(0, 0.0005, 3)]) for _ in range(B)]
    frames = torch.from_numpy(np.stack([s.frame(1)] * B)).cuda()
    ipts = np.stack([s.corners(1) + rng.normal(0, 0.1, (48, 2)).astype(np.float32) for _ in range(B)])
    mask = (rng.uniform(size=(B, 48)) > 0.2).astype(np.uint8)
    ctx = cv_hip.Context(64, 64, max_level=0)
    for (iters, pw, with_corners) in ((1, 1.0, False), (6, 1.0, False), (6, 0.01, True)):
        pose = torch.from_numpy(np.stack(starts)).cuda().contiguous()
        kw = dict(obj=torch.from_numpy(s.obj.astype(np.float32)).cuda(), img_pts=torch.from_numpy(ipts).cuda().contiguous(),
                  mask=torch.from_numpy(mask).cuda().contiguous()) if with_corners else {}
        pose, stats = ctx.dense_refine(frames, torch.from_numpy(mx).cuda(), torch.from_numpy(T).cuda(), pose, s.K, dist,
                                       iters=iters, photo_weight=pw, **kw)
        pose, stats = pose.cpu().numpy(), stats.cpu().numpy()
        for b in range(B):
            r, t, st = oracle.dense_refine(s.frame(1), mx, T, s.obj if with_corners else None, ipts[b] if with_corners else None,
                                           mask[b] if with_corners else None, s.K, dist, starts[b][:3], starts[b][3:], iters=iters, photo_weight=pw)
            assert np.abs(pose[b, :3] - r).max() < 1e-9 and np.abs(pose[b, 3:] - t).max() < 1e-9
            assert int(stats[b, 2]) == st["valid"] and int(stats[b, 3]) == st["iters"] and int(stats[b, 4]) == st["used"]
            assert abs(stats[b, 0] - st["photo_rms"]) < 1e-8 and abs(stats[b, 1] - st["geo_rms"]) < 1e-8


@pytest.mark.gpu
def test_config5_sizes_240_corners_61440_samples(oracle):
    """BASELINE configs[4]: 60 tags / 240 corners + 60 x 32 x 32 dense samples on a 1280x720 frame"""
    import torch
    from accurate_aprilgroup_tracking_amd import cv_hip
    s = syn.Sequence(1280, 720, n_tags=60, n_frames=2, seed=8, supersample=2)
    mx = syn.model_samples(s.group, 32)
    assert mx.shape[0] == 61440 and s.obj.shape[0] == 240
    T = np.nan_to_num(syn.sample_bilinear(s.frame(1), syn.project(mx, s.rvecs[1], s.tvecs[1], s.K)), nan=128.0).astype(np.float32)
    start = np.concatenate([s.rvecs[1] + 0.002, s.tvecs[1] - 0.0006])
    ctx = cv_hip.Context(64, 64, max_level=0)
    pose = torch.from_numpy(start[None].copy()).cuda()
    pose, stats = ctx.dense_refine(torch.from_numpy(s.frame(1)[None]).cuda(), torch.from_numpy(mx).cuda(), torch.from_numpy(T).cuda(), pose,
                                   s.K, None, obj=torch.from_numpy(s.obj.astype(np.float32)).cuda(),
                                   img_pts=torch.from_numpy(s.corners(1)[None]).cuda().contiguous(), iters=8, photo_weight=0.05)
    pose = pose.cpu().numpy()[0]
    r, t, st = oracle.dense_refine(s.frame(1), mx, T, s.obj, s.corners(1), None, s.K, None, start[:3], start[3:], iters=8, photo_weight=0.05)
    assert np.abs(pose[:3] - r).max() < 1e-9 and np.abs(pose[3:] - t).max() < 1e-9
    assert np.abs(pose[:3] - s.rvecs[1]).max() < 1e-4 and np.abs(pose[3:] - s.tvecs[1]).max() < 1e-4
    assert stats.cpu().numpy()[0, 4] == 240


@pytest.mark.gpu
def test_scratch_survives_undistort_init_and_batch_growth(oracle, scene):
    """(1) agt_undistort_init must not touch the dense scratch (it freed it without resetting the capacity);
    (2) the per-stream done words have their own capacity: B = 1 with many samples followed by B = 64 with few."""
    import torch
    from accurate_aprilgroup_tracking_amd import cv_hip
    s, mx = scene
    T = _template(s, mx, 1)
    start = np.concatenate([s.rvecs[1] + 0.002, s.tvecs[1] - 0.0004])
    want_r, want_t, _ = oracle.dense_refine(s.frame(1), mx, T, None, None, None, s.K, None, start[:3], start[3:], iters=4, photo_weight=1.0)
    ctx = cv_hip.Context(s.width, s.height, max_level=0)
    mxg, Tg = torch.from_numpy(mx).cuda(), torch.from_numpy(T).cuda()

    def run(B, m=None):
        frames = torch.from_numpy(np.stack([s.frame(1)] * B)).cuda()
        pose = torch.from_numpy(np.repeat(start[None], B, 0).copy()).cuda()
        a, b = (mxg, Tg) if m is None else (mxg[:m].contiguous(), Tg[:m].contiguous())
        pose, _ = ctx.dense_refine(frames, a, b, pose, s.K, None, iters=4, photo_weight=1.0)
        return pose.cpu().numpy()

    def check(p):
        assert np.abs(p[:, :3] - want_r).max() < 1e-9 and np.abs(p[:, 3:] - want_t).max() < 1e-9

    check(run(1))
    ctx.undistort_init(s.K, syn.MILD_DIST, None, s.width, s.height)        # first map build: map size changes from 0
    m1 = ctx.undistort_maps()[0].copy()
    check(run(1))
    ctx.undistort_init(s.K, syn.MILD_DIST, None, s.width, s.height)
    assert np.array_equal(ctx.undistort_maps()[0], m1)                        # maps were not clobbered by the dense scratch
    small = run(64, 256)                                                   # more streams, fewer samples than the first call
    r, t, _ = oracle.dense_refine(s.frame(1), mx[:256], T[:256], None, None, None, s.K, None, start[:3], start[3:], iters=4, photo_weight=1.0)
    assert np.abs(small[:, :3] - r).max() < 1e-9 and np.abs(small[:, 3:] - t).max() < 1e-9
    check(run(1))


@pytest.mark.gpu
@pytest.mark.parametrize("reseed,cam", [(False, "pinhole"), (True, "pinhole"), (True, "tilt")])
def test_c5_stream_matches_oracle_chain(oracle, reseed, cam, tmp_path):
    """BASELINE configs[4] as a STREAM: 1280x720, 60 tags / 240 corners, 61,440 dense samples.  Every frame runs
    LK(240) -> solvePnP(240, guess) + gate + motion model -> dense refinement of the accepted pose (-> corner re-seed)
    on the device with no host round trip (StreamTracker.step_dense); the CPU chain is the oracle LK (sticky status), the
    reference-validated PoseDetector mirror on the oracle backend and oracle.dense_refine, frame by frame.
    cam = "tilt" (round 5): the same chain through the 14-coefficient model with a (small) sensor tilt -- solver, dense stage and the
    re-seed's projection all go through the tilted projection; the frames are the renderer's (no tilt), so only HIP = oracle is asserted."""
    _c5_chain(oracle, reseed, cam, tmp_path, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("reseed", [False, True], ids=["L3", "L3_reseed"])
def test_c5_stream_matches_oracle_chain_at_depth_3(oracle, reseed, tmp_path):
    """the same chain with pyramids of depth 3 on both sides: LK(240) and the cooperative pose solve go out as ONE launch of the
    six-level kernel (agt_step_dense.hip lk_pnp_coop_kernel<6>)"""
    _c5_chain(oracle, reseed, "pinhole", tmp_path, 3)


def _c5_chain(oracle, reseed, cam, tmp_path, max_level):
    dist = TILT14 if cam == "tilt" else None
    import json, logging
    import torch
    from oracle import cv2_shim
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = syn.Sequence(1280, 720, n_tags=60, n_frames=6, seed=8, supersample=2)
    n = s.obj.shape[0]
    assert n == 240 and s.coverage(0).max() <= 1.0 + 1e-6           # no two tags overlap in the image
    mx = syn.model_samples(s.group, 32)
    T = _template(s, mx, 0)                                         # template captured at the initial (known) pose
    iters, pw = 4, 0.05
    tol = 1e-6 if reseed else 1e-8        # re-seeded corners are rounded to float32: an ulp flip costs ~1e-7 downstream
    F = len(s)
    frames = torch.from_numpy(s.frames()).cuda()
    trk = StreamTracker(s.width, s.height, s.obj, s.K, dist, n_streams=1, max_level=max_level)
    assert trk.ctx.eff_max_level == max_level
    mxg, Tg = torch.from_numpy(mx).cuda(), torch.from_numpy(T).cuda()
    trk.dense_model(mxg, Tg, iters=iters, photo_weight=pw, reseed=reseed)
    trk.reset(frames[0:1].contiguous(), torch.from_numpy(s.corners(0)[None]).cuda().contiguous())
    so = trk.new_state_buffer(F - 1)
    do = torch.zeros((F - 1, 1, H.DENSE_STRIDE), dtype=torch.float64, device="cuda")
    for k in range(1, F):
        trk.step_dense(frames[k:k + 1], so[k - 1], do[k - 1])        # never synchronised in between
    torch.cuda.synchronize()
    st, dn = so.cpu().numpy()[:, 0], do.cpu().numpy()[:, 0]

    (tmp_path / "april_group.json").write_text(json.dumps(s.group))

    class Det(PoseDetector):
        DIRPATH = str(tmp_path)
    log = logging.getLogger("c5"); log.setLevel(logging.CRITICAL)
    det = Det(log, s.K, dist, True, cv=cv2_shim.make_cv2())
    obj32 = s.obj.astype(np.float32)
    pts = s.corners(0); alive = np.ones(n, bool); pyr = oracle.Pyramid(s.frame(0), 21, max_level)
    assert pyr.levels == max_level
    for k in range(1, F):
        npyr = oracle.Pyramid(s.frame(k), 21, max_level)
        nx, status, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, maxLevel=max_level)
        if k == 1 and max_level != 2:
            # the scene tells the depth from depth 2: some corner lands elsewhere
            n2, _, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, maxLevel=2)
            assert (n2.view(np.uint32) != nx.view(np.uint32)).any()
        nx = nx.reshape(-1, 2); status = status.ravel().astype(bool)
        nx[~alive] = pts[~alive]; alive &= status
        il = [nx[i].reshape(1, 1, 2) for i in range(n) if alive[i]]
        ol = [obj32[i].reshape(1, 3) for i in range(n) if alive[i]]
        det._estimate_pose(il if len(il) >= 8 else [], ol if len(il) >= 8 else [])
        accepted = det.last_error is not None and det.last_error < 2
        assert int(st[k - 1, H.ST_NTRACK]) == int(alive.sum()) and int(st[k - 1, H.ST_OK]) == int(accepted)
        assert accepted and alive.sum() == n, "the 60-tag scene keeps all 240 corners trackable"
        r0 = det.last_pose[0].ravel().astype(np.float64); t0 = det.last_pose[1].ravel().astype(np.float64)
        assert np.abs(st[k - 1, :3] - r0).max() < tol and np.abs(st[k - 1, 3:6] - t0).max() < tol, "frame %d PnP pose" % k
        r, t, info = oracle.dense_refine(s.frame(k), mx, T, s.obj, nx.astype(np.float32), alive.astype(np.uint8), s.K, dist, r0, t0,
                                         iters=iters, photo_weight=pw)
        assert dn[k - 1, H.DN_REFINED] == 1.0
        assert np.abs(dn[k - 1, :3] - r).max() < tol and np.abs(dn[k - 1, 3:6] - t).max() < tol, "frame %d refined pose" % k
        assert int(dn[k - 1, H.DN_VALID]) == info["valid"] and int(dn[k - 1, H.DN_ITERS]) == info["iters"] and int(dn[k - 1, H.DN_CORNERS]) == info["used"]
        assert abs(dn[k - 1, H.DN_PHOTO_RMS] - info["photo_rms"]) < 1e-5 and abs(dn[k - 1, H.DN_GEO_RMS] - info["geo_rms"]) < 1e-5
        # the refinement must not be worse than the PnP pose against the generator's truth
        e_pnp = max(np.abs(r0 - s.rvecs[k]).max(), np.abs(t0 - s.tvecs[k]).max())
        e_ref = max(np.abs(r - s.rvecs[k]).max(), np.abs(t - s.tvecs[k]).max())
        assert cam == "tilt" or (e_ref < 2e-3 and e_ref < e_pnp + 2e-4)
        if reseed:
            pp, _ = oracle.projectPoints(s.obj, r, t, s.K, dist)
            pts = pp.reshape(-1, 2).astype(np.float32); alive[:] = True
        else:
            pts = nx.astype(np.float32)
        pyr = npyr


@pytest.mark.gpu
@pytest.mark.parametrize("n_tags,reseed", [(60, True), (12, True), (60, False), (12, False)])
def test_dense_clip_submission_equals_single_calls(oracle, n_tags, reseed):
    """agt_track_frames_dense (include/agt_hip.h): a clip of frames in one call -- the pyramid pass of frame k + 1 rides in a
    launch of frame k: the four-wave PnP launch (240 corners) or the second dense launch (48 corners) -- leaves bitwise the
    records of agt_track_frame_dense called frame by frame; clips cut at arbitrary places, a clip of one frame, a single call
    between two clips."""
    _dense_clip_equals_single_calls(n_tags, reseed, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("n_tags,reseed", [(60, True), (12, True), (60, False), (12, False)], ids=["L3-60-reseed", "L3-12-reseed", "L3-60", "L3-12"])
def test_dense_clip_submission_equals_single_calls_at_depth_3(oracle, n_tags, reseed):
    """the same at pyramid depth 3, where no pyramid pass rides (that form is built for depth 2): the clip form differs from the single
    calls only by the deferred last dense step -- lk_pnp_coop_kernel<6> takes it as its prologue with 240 corners, lk_reseed_kernel<6>
    with 48"""
    _dense_clip_equals_single_calls(n_tags, reseed, 3)


def _dense_clip_equals_single_calls(n_tags, reseed, max_level):
    import torch
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = syn.Sequence(1280, 720, n_tags=n_tags, n_frames=6, seed=8, supersample=2)
    mx = syn.model_samples(s.group, 32 if n_tags == 60 else 16)
    T = _template(s, mx, 0)
    frames = torch.from_numpy(s.frames()).cuda()
    order = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0, 1, 2]
    clip = frames[order].unsqueeze(1).contiguous()                       # [K, 1, H, W]
    K = len(order)
    outs = []
    for cuts in (None, [K], [1, 4, 1, 6], [5, 0, 6]):
        trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=1, max_level=max_level)
        assert trk.ctx.eff_max_level == max_level
        trk.dense_model(torch.from_numpy(mx).cuda(), torch.from_numpy(T).cuda(), iters=4, photo_weight=0.05, reseed=reseed)
        trk.reset(frames[0:1].contiguous(), torch.from_numpy(s.corners(0)[None]).cuda().contiguous())
        so = trk.new_state_buffer(K)
        do = torch.zeros((K, 1, H.DENSE_STRIDE), dtype=torch.float64, device="cuda")
        if cuts is None:
            for k in range(K):
                trk.step_dense(clip[k], so[k], do[k])
        else:
            k = 0
            for m in cuts:
                if m == 0:                      # a single call between two clips
                    trk.step_dense(clip[k], so[k], do[k]); k += 1
                else:
                    trk.step_many_dense(clip[k:k + m], so[k:k + m], do[k:k + m]); k += m
            assert k == K
        torch.cuda.synchronize()
        outs.append((so.cpu().numpy().copy(), do.cpu().numpy().copy()))
    st0, dn0 = outs[0]
    assert st0[:, 0, H.ST_OK].all() and (dn0[:, 0, H.DN_REFINED] == 1.0).all()
    for st, dn in outs[1:]:
        assert np.array_equal(st.view(np.uint64), st0.view(np.uint64)) and np.array_equal(dn.view(np.uint64), dn0.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("B2_240_reseed_prologue", 60, 2), ("B2_96_chained", 24, 2), ("B2_120_chained", 30, 2), ("B1_240_chained", 60, 1)],
                         ids=lambda c: c[0])
def test_dense_clip_with_rejected_and_lost_frames_equals_single_calls(oracle, case):
    """The clip form's launches (include/agt_hip.h agt_track_frames_dense) against agt_track_frame_dense called frame by frame, on
    streams of which one sees a frame of another sequence (the gate rejects: done word set, no refinement, no re-seed)
    and later a blank frame (LK loses every corner for good): records, corner sets and LK status bitwise equal, whatever the cuts.
    WHICH launch form a case reaches (the 240-corner B = 2 case of round 4 never reached the chained kernel --
    2 x 240 + 2 workgroups do not fit the chip at one per CU):
      B2_240  lk_reseed_kernel: the previous frame's final update + re-seed as the LK launch's prologue, PnP a launch of its own;
      B2_96 / B2_120 / B1_240  lk_pnp_coop_kernel: LK and the four-wave PnP CHAINED in one launch (64 < n <= 256 corners and
              n B + B <= 256 workgroups) -- per-stream indexing of the solver workgroups (b = blockIdx.x - n_lk, wait[0] + b,
              track[b], the riding pyramid tiles' stream index) with two DISTINCT streams, gate-rejected frames and frames in
              which every corner is lost, in the chained kernel itself."""
    import ctypes as C
    import torch
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    _, n_tags, B = case
    seqs = [syn.Sequence(1280, 720, n_tags=n_tags, n_frames=8, seed=8 + i, supersample=2, group_seed=8) for i in range(2)]
    s = seqs[0]
    n = s.obj.shape[0]
    mx = syn.model_samples(s.group, 16)
    T = _template(s, mx, 0)
    fr = [sq.frames() for sq in seqs]
    order0 = [1, 2, 3, 4, 5, 6, 7, 6, 5, 4]
    order1 = [1, 2, 7, 3, 4, 5, -1, 6, 7, 6]          # the disturbed stream: entry 2 is replaced below, entry 6 is a blank frame
    K = len(order0)
    blank = np.full((720, 1280), 128, np.uint8)
    dist_frames = [blank if order1[k] < 0 else fr[1][order1[k]] for k in range(K)]
    dist_frames[2] = fr[0][4]                         # a frame of the OTHER sequence: LK lands ~9 px off any pose of the model (CPU oracle: mean error 8.6-9.7 px), the gate rejects
    if B == 2:
        clip = np.stack([np.stack([fr[0][order0[k]], dist_frames[k]]) for k in range(K)])
        first = np.stack([fr[0][0], fr[1][0]]); c0 = np.stack([seqs[0].corners(0), seqs[1].corners(0)])
    else:
        clip = np.stack([dist_frames[k][None] for k in range(K)])
        first = fr[1][0][None]; c0 = seqs[1].corners(0)[None]
    clip = torch.from_numpy(clip).cuda().contiguous()                    # [K, B, H, W]
    first = torch.from_numpy(first).cuda().contiguous()
    c0 = torch.from_numpy(c0).cuda().contiguous()
    outs = []
    for cuts in (None, [K], [3, 1, 6], [2, 0, 5, 0, 1]):
        trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=B)
        trk.dense_model(torch.from_numpy(mx).cuda(), torch.from_numpy(T).cuda(), iters=3, photo_weight=0.05, reseed=True)
        trk.reset(first, c0)
        so = trk.new_state_buffer(K)
        do = torch.zeros((K, B, H.DENSE_STRIDE), dtype=torch.float64, device="cuda")
        if cuts is None:
            for k in range(K):
                trk.step_dense(clip[k], so[k], do[k])
        else:
            k = 0
            for m in cuts:
                if m == 0:
                    trk.step_dense(clip[k], so[k], do[k]); k += 1
                else:
                    trk.step_many_dense(clip[k:k + m], so[k:k + m], do[k:k + m]); k += m
            assert k == K
        torch.cuda.synchronize()
        cp, sp = trk.corners()                                           # device addresses of the newest frame's corner set / LK status
        pts, status = np.zeros((B, n, 2), np.float32), np.zeros((B, n), np.uint8)
        H.check(trk.ctx.L.agt_download(trk.ctx.h, pts.ctypes.data_as(C.c_void_p), C.c_void_p(cp), pts.nbytes), "agt_download")
        H.check(trk.ctx.L.agt_download(trk.ctx.h, status.ctypes.data_as(C.c_void_p), C.c_void_p(sp), status.nbytes), "agt_download")
        outs.append((so.cpu().numpy().copy(), do.cpu().numpy().copy(), pts, status))
    st0, dn0, p0, u0 = outs[0]
    d = B - 1                                                            # index of the disturbed stream
    if B == 2:
        assert st0[:, 0, H.ST_OK].all() and (dn0[:, 0, H.DN_REFINED] == 1.0).all()          # the undisturbed stream
    assert st0[:2, d, H.ST_OK].all() and not st0[2, d, H.ST_OK], "the jump frame's pose is rejected by the gate"
    assert dn0[2, d, H.DN_REFINED] == 0.0
    assert not st0[6:, d, H.ST_OK].any() and (dn0[6:, d, H.DN_REFINED] == 0.0).all()        # from the blank frame on: nothing tracked, nothing refined
    assert (st0[7:, d, H.ST_NTRACK] == 0).all()           # (the frame AFTER the blank one: its previous patches are flat)
    for st, dn, p, u in outs[1:]:
        assert np.array_equal(st.view(np.uint64), st0.view(np.uint64)) and np.array_equal(dn.view(np.uint64), dn0.view(np.uint64))
        assert np.array_equal(p.view(np.uint32), p0.view(np.uint32)) and np.array_equal(u, u0)


_DENSE_GIVE_UP_CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, os.environ["AGT_REPO_ROOT"])
import torch
from accurate_aprilgroup_tracking_amd import hiplib as H
H.LIB_PATH = os.path.join(os.path.dirname(H.LIB_PATH), "libagt_hip_dbg.so")
from accurate_aprilgroup_tracking_amd import synthetic as syn
from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
s = syn.Sequence(1280, 720, n_tags=60, n_frames=6, seed=8, supersample=2)
mx = syn.model_samples(s.group, 16)
T = np.nan_to_num(syn.sample_bilinear(s.frame(0), syn.project(mx, s.rvecs[0], s.tvecs[0], s.K)), nan=128.0).astype(np.float32)
frames = torch.from_numpy(s.frames()).cuda()
order = [1, 2, 3, 4, 5, 4, 3, 2]
clip = frames[order].unsqueeze(1).contiguous()
trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=1)
trk.dense_model(torch.from_numpy(mx).cuda(), torch.from_numpy(T).cuda(), iters=3, photo_weight=0.05, reseed=True)
out = {}
def run(tag):
    trk.reset(frames[0:1].contiguous(), torch.from_numpy(s.corners(0)[None]).cuda().contiguous())
    so = trk.new_state_buffer(len(order))
    do = torch.zeros((len(order), 1, H.DENSE_STRIDE), dtype=torch.float64, device="cuda")
    trk.step_many_dense(clip, so, do)
    code = trk.ctx.L.agt_synchronize(trk.ctx.h)
    out[tag] = dict(st=so.cpu().numpy()[:, 0].tolist(), dn=do.cpu().numpy()[:, 0].tolist(), code=code, chain_fault=trk.read_state()[0].chain_fault)
run("faulted")          # AGT_CHAIN_WITHHOLD_DENSE=3: the third chained LK | PnP launch never sees its last arrival
run("recovered")        # the knob has fired; agt_tracker_reset brings the stream back
print("RESULT " + json.dumps(out))
'''


@pytest.mark.gpu
def test_dense_chained_launch_give_up_is_fail_stop(oracle):
    """The chained LK | PnP launch of dense clips (agt_step.hip lk_pnp_coop_kernel) when an arrival never comes (diagnostic library,
    AGT_CHAIN_WITHHOLD_DENSE): the solver's workgroup gives up after its poll budget, the frame's record is flagged
    AGT_TRK_CHAIN_TIMEOUT and zero, its dense record unrefined, every later record of the stream flagged too; the clip DRAINS (no
    hang), agt_synchronize reports AGT_ERR_CHAIN, agt_tracker_reset recovers: the records of a clean run, bit for bit."""
    import json
    import subprocess
    import sys
    import torch
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dbg = os.path.join(root, "accurate_aprilgroup_tracking_amd", "libagt_hip_dbg.so")
    if not os.path.exists(dbg):
        subprocess.check_call(["make", "-s", "-j", "8", "-C", os.path.join(root, "accurate_aprilgroup_tracking_amd", "csrc"), "dbg"])
    env = dict(os.environ, AGT_CHAIN_WITHHOLD_DENSE="3", AGT_REPO_ROOT=root)
    res = subprocess.run([sys.executable, "-c", _DENSE_GIVE_UP_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.loads([l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    f, r = out["faulted"], out["recovered"]
    st, dn = np.array(f["st"]), np.array(f["dn"])
    flags = st[:, H.ST_FLAGS].astype(int)
    bad = np.nonzero(flags & H.TRK_CHAIN_TIMEOUT)[0]
    assert len(bad) and int(bad[0]) == 2, "the withheld arrival belongs to the third chained launch"
    assert np.array_equal(bad, np.arange(2, len(st))), "every record after the give-up is flagged (sticky fault)"
    assert (st[2:, :8] == 0).all() and (dn[2:, H.DN_REFINED] == 0).all(), "nothing is solved or refined on the faulted frames"
    assert st[:2, H.ST_OK].all() and (dn[:2, H.DN_REFINED] == 1).all()
    assert f["code"] == -8 and f["chain_fault"] == 1, "agt_synchronize reports AGT_ERR_CHAIN"
    rs, rd = np.array(r["st"]), np.array(r["dn"])
    assert r["code"] == 0 and r["chain_fault"] == 0 and rs[:, H.ST_OK].all() and (rd[:, H.DN_REFINED] == 1).all()
    assert np.array_equal(rs[:2], st[:2]) and np.array_equal(rd[:2], dn[:2]), "the frames before the give-up were those of the clean run"


def test_synthetic_60_tag_layout():
    """the 60-tag model of configs[4]: every tag inside a 1280x720 frame along the trajectory, none overlapping another"""
    s = syn.Sequence(1280, 720, n_tags=60, n_frames=120, seed=8, supersample=1)
    assert s.obj.shape == (240, 3)
    for k in (0, 40, 80, 119):
        c = s.corners(k)
        assert c[:, 0].min() > 12 and c[:, 0].max() < 1280 - 12 and c[:, 1].min() > 12 and c[:, 1].max() < 720 - 12
        assert s.coverage(k).max() <= 1.0 + 1e-6
