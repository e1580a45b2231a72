"""-m gpu: the visibility rule of the reproject refresh on the device -- agt_tag_visibility against the numpy rule, the tracker against
its CPU chain on a closed body, what the rule is for, and how it composes (off, 90 degrees on the cap, the dense refusal, the
forward-backward check).

Expected values: tests/visibility_scenes.py -- `tag_visibility` (numpy float64 on `oracle.Rodrigues`) and `oracle_chain` (oracle LK +
the PoseDetector mirror on the oracle backend + the refresh in Python).  The scenes and the numpy rule are checked on the CPU in
tests/test_tag_visibility.py.

Figures of test_the_rule_keeps_the_pose_on_the_turning_body (24 tags, +2 degrees per frame, rotation gap to the truth at frame 15):
CPU chain of tools/visibility_drift.py 0.071 rad with the rule at 70 degrees against 0.511 rad without; the device's are printed by the
test and filed in profiles/tag_visibility.md.
"""
import ctypes as C

import numpy as np
import pytest

import visibility_scenes as S

pytestmark = pytest.mark.gpu
COS_TOL = 1e-9           # the project's FP64 parity bound for pose arithmetic
POSE_TOL = 1e-6          # reproject rounds the refreshed corners to float32 (test_fused_track_frame_matches_oracle_chain)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


@pytest.fixture(scope="module")
def chains(oracle, tmp_path_factory):
    """the oracle chains of the tracker tests, computed once: (tags, step, view_deg, fb_px) -> records"""
    tmp = tmp_path_factory.mktemp("vis")
    memo = {}

    def get(n_tags, step, view_deg, fb_px=0.0):
        key = (n_tags, step, view_deg, fb_px)
        if key not in memo:
            memo[key] = S.oracle_chain(oracle, S.ClosedBodyClip.get(n_tags, step), tmp, "c%d_%g_%g_%g" % key, view_deg, fb_px)
        return memo[key]
    return get


# ------------------------------------------------------------------------------------------------------- the stand-alone call
def _poses(n_tags):
    """B = 5 seeded poses around the clip's; the last one puts the body behind the camera (every tag centre has c_c.z <= 0)"""
    rng = np.random.default_rng(100 + n_tags)
    r = np.asarray(S.R0) + rng.uniform(-1.2, 1.2, (5, 3))
    t = np.asarray(S.T0) + rng.uniform(-0.03, 0.03, (5, 3))
    t[4] = (0.01, -0.01, -0.25)
    return np.concatenate([r, t], axis=1)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n_tags", [12, 24])
def test_tag_visibility_against_the_numpy_rule(torch_cuda, oracle, n_tags, dtype):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import cv_hip
    clip = S.ClosedBodyClip.get(n_tags)
    npdt = np.float32 if dtype == "f32" else np.float64
    poses = _poses(n_tags)
    B, T = poses.shape[0], n_tags
    shared = np.ascontiguousarray(clip.obj.astype(npdt))
    # per-stream object points: the same body, a little larger and shifted from stream to stream
    own = np.ascontiguousarray(np.stack([clip.obj * (1.0 + 0.02 * b) + 0.001 * b for b in range(B)]).astype(npdt))
    ctx = cv_hip.Context(64, 64, max_level=0)
    pg = torch.from_numpy(poses).cuda().contiguous()
    behind = 0
    for name, objs in (("shared", shared), ("per-stream", own)):
        og = torch.from_numpy(objs).cuda().contiguous()
        for deg in (60.0, 75.0, 90.0):
            for facing in (1, -1):
                ref = [S.tag_visibility(objs if objs.ndim == 2 else objs[b], poses[b, :3], poses[b, 3:], 4, deg, facing) for b in range(B)]
                rv = np.stack([r[0] for r in ref]); rc = np.stack([r[1] for r in ref]); rz = np.stack([r[2] for r in ref])
                # no tag is left out: every reference cosine is clear of the threshold
                assert np.abs(rc - S.cos_threshold(deg)).min() > 1e-6
                vis, cs = ctx.tag_visibility(og, pg, 4, deg, facing)
                torch.cuda.synchronize()
                vis, cs = vis.cpu().numpy(), cs.cpu().numpy()
                where = "%d tags %s %s %g deg facing %d" % (n_tags, dtype, name, deg, facing)
                assert vis.shape == (B, T) and cs.shape == (B, T)
                assert np.abs(cs - rc).max() <= COS_TOL, where + ": cos differs by %g" % np.abs(cs - rc).max()
                assert np.array_equal(vis.astype(bool), rv), where + ": flags"
                assert (rz[4] <= 0).all() and not vis[4].any(), where + ": a tag behind the camera is hidden"
                behind += int(((rz[4] <= 0) & (rc[4] > S.cos_threshold(deg))).sum())
                assert rv[:4].any() and not rv[:4].all()
                # without the cosine output
                vis2, none = ctx.tag_visibility(og, pg, 4, deg, facing, want_cos=False)
                assert none is None and np.array_equal(vis2.cpu().numpy(), vis)
    assert behind > 0, "no tag behind the camera was hidden by its depth alone"


def test_tag_visibility_cv_call_and_argument_errors(torch_cuda, oracle):
    from accurate_aprilgroup_tracking_amd import cv_hip, hiplib as H
    torch = torch_cuda
    clip = S.ClosedBodyClip.get(24)
    for k, deg, facing in ((0, 90.0, 1), (9, 70.0, 1), (15, 75.0, -1)):
        vis, cs = cv_hip.tagVisibility(clip.obj, clip.rvecs[k], clip.tvecs[k].reshape(3, 1), maxViewDeg=deg, facing=facing)
        rv, rc, _ = S.tag_visibility(clip.obj, clip.rvecs[k], clip.tvecs[k], 4, deg, facing)
        assert vis.dtype == bool and vis.shape == (24,) and cs.dtype == np.float64 and cs.shape == (24,)
        assert np.array_equal(vis, rv) and np.abs(cs - rc).max() <= COS_TOL
    ctx = cv_hip.Context(64, 64, max_level=0)
    obj = torch.from_numpy(clip.obj).cuda().contiguous()
    pose = torch.from_numpy(clip.truth(0)[None]).cuda().contiguous()
    for kw in (dict(max_view_deg=0.0), dict(max_view_deg=-1.0), dict(max_view_deg=91.0), dict(max_view_deg=float("nan")),
               dict(max_view_deg=float("inf")), dict(facing=0), dict(facing=3)):
        with pytest.raises(H.AgtError) as e:
            ctx.tag_visibility(obj, pose, **kw)
        assert e.value.code == -1
    with pytest.raises(cv_hip.error):
        ctx.tag_visibility(obj, pose, corners_per_tag=5)


# ------------------------------------------------------------------------------------------------------------------- tracker
class DeviceRun:
    """B closed-body clips of one body through ONE StreamTracker under reproject: frame 0 detector-fed with the clip's seed mask,
    frames 1.. tracked.  rec [F, B, 16], status [F, B, n] (the status table after every frame), corners [B, n, 2] (final)."""

    def __init__(self, clips, view_deg=0.0, fb_px=0.0, facing=1, seed_deg=None):
        import torch
        from accurate_aprilgroup_tracking_amd import hiplib as H
        from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
        c0 = clips[0]
        B, n, F = len(clips), c0.obj.shape[0], len(c0)
        seed_deg = seed_deg or view_deg or S.VIEW_DEG[c0.n_tags]
        frames = [torch.from_numpy(np.stack([c.frame(k) for c in clips])).cuda().contiguous() for k in range(F)]
        corners0 = torch.from_numpy(np.stack([c.corners(0) for c in clips])).cuda().contiguous()
        mask0 = torch.from_numpy(np.stack([c.seed_mask(seed_deg) for c in clips])).cuda().contiguous()
        trk = StreamTracker(c0.width, c0.height, c0.obj, c0.K, None, n_streams=B, reproject=True, fb_check=fb_px, view_deg=view_deg, facing=facing)
        trk.reset()
        so = torch.zeros((F, B, H.STATE_STRIDE), dtype=torch.float64, device="cuda")
        self.status = np.zeros((F, B, n), np.uint8)
        self.corners = np.zeros((B, n, 2), np.float32)
        for k in range(F):
            if k == 0:
                trk.step_detected(frames[0], corners0, mask0, so[0])
            else:
                trk.step(frames[k], so[k])
            trk.join()
            torch.cuda.synchronize()
            cp, sp = trk.corners()
            H.check(trk.ctx.L.agt_download(trk.ctx.h, self.status[k].ctypes.data_as(C.c_void_p), C.c_void_p(sp), self.status[k].nbytes), "agt_download")
        H.check(trk.ctx.L.agt_download(trk.ctx.h, self.corners.ctypes.data_as(C.c_void_p), C.c_void_p(cp), self.corners.nbytes), "agt_download")
        self.rec = so.cpu().numpy()
        assert not (self.rec[:, :, H.ST_FLAGS].astype(int) & H.TRK_CHAIN_TIMEOUT).any()


def _assert_chain(run, b, recs, what):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    for k, r in enumerate(recs):
        g = run.rec[k, b]
        where = "%s stream %d frame %d" % (what, b, k)
        assert int(g[H.ST_NTRACK]) == r["ntrack"], where + ": tracked corners %d, chain %d" % (g[H.ST_NTRACK], r["ntrack"])
        assert bool(g[H.ST_OK]) == r["ok"], where + ": acceptance"
        assert int(g[H.ST_NVISIBLE]) == r["nvisible"], where + ": visible tags %d, chain %d" % (g[H.ST_NVISIBLE], r["nvisible"])
        if r["pose"] is not None:
            assert np.abs(g[:6] - r["pose"]).max() <= POSE_TOL, where + ": pose differs by %g" % np.abs(g[:6] - r["pose"]).max()
        assert np.array_equal(run.status[k, b].astype(bool), r["status"]), where + ": status table, device %s chain %s" % (
            np.nonzero(run.status[k, b])[0], np.nonzero(r["status"])[0])


def _assert_scene_works(recs, view_deg, what):
    """the run-time conditions on the oracle chain: no verdict near the threshold, enough tags, tags entering and leaving"""
    assert min(r["margin"] for r in recs) > 1e-4, what + ": a refresh cosine within 1e-4 of the threshold"
    assert all(r["ok"] for r in recs), what + ": the chain rejects a frame"
    assert min(r["nvisible"] for r in recs) >= 3, what
    tags = np.stack([r["status"].reshape(-1, 4).all(axis=1) for r in recs])
    enter, leave = int((tags[1:] & ~tags[:-1]).sum()), int((~tags[1:] & tags[:-1]).sum())
    assert enter >= 1 and leave >= 1, what + ": %d entries, %d exits" % (enter, leave)


@pytest.mark.parametrize("n_tags", [12, 24], ids=["one_wave_48", "coop_96"])
def test_tracker_with_the_rule_matches_its_oracle_chain(torch_cuda, chains, n_tags):
    """stream 0 turns by +2 degrees per frame, stream 1 by -2: two different visible sets in every launch"""
    deg = S.VIEW_DEG[n_tags]
    steps = (S.STEP_DEG, -S.STEP_DEG)
    want = [chains(n_tags, s, deg) for s in steps]
    for b, recs in enumerate(want):
        _assert_scene_works(recs, deg, "%d tags, step %g" % (n_tags, steps[b]))
    assert any(not np.array_equal(a["status"], c["status"]) for a, c in zip(*want)), "the two streams hold the same visible sets"
    run = DeviceRun([S.ClosedBodyClip.get(n_tags, s) for s in steps], deg)
    for b, recs in enumerate(want):
        _assert_chain(run, b, recs, "%d tags at %g deg" % (n_tags, deg))


def test_the_rule_keeps_the_pose_on_the_turning_body(torch_cuda):
    """What the rule is for: 24 tags, +2 degrees per frame, device only.  The plain refresh revives the far side, whose corners track
    front-side texture, and the pose stops following the body; with the rule it does not."""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    clip = S.ClosedBodyClip.get(24, S.STEP_DEG)
    deg = S.VIEW_DEG[24]
    plain = DeviceRun([clip], 0.0, seed_deg=deg)
    ruled = DeviceRun([clip], deg)
    last = len(clip) - 1
    gap_plain = S.rotation_gap(plain.rec[last, 0, :3], clip.rvecs[last])
    gap_ruled = S.rotation_gap(ruled.rec[last, 0, :3], clip.rvecs[last])
    print("rotation gap to the truth at frame %d: plain refresh %.4f rad, rule at %g degrees %.4f rad (ratio %.3f); reprojection error "
          "plain %.2f-%.2f px, ruled %.2f-%.2f px" % (last, gap_plain, deg, gap_ruled, gap_ruled / gap_plain,
                                                       plain.rec[:, 0, H.ST_ERR].min(), plain.rec[:, 0, H.ST_ERR].max(),
                                                       ruled.rec[:, 0, H.ST_ERR].min(), ruled.rec[:, 0, H.ST_ERR].max()))
    assert (plain.rec[:, 0, H.ST_OK] == 1).all() and (ruled.rec[:, 0, H.ST_OK] == 1).all(), "a frame was rejected"
    assert (plain.rec[:, 0, H.ST_NVISIBLE] == 0).all() and plain.status[last].all(), "the plain refresh revives every corner"
    assert gap_ruled <= 0.5 * gap_plain, "plain %.4f rad, with the rule %.4f rad" % (gap_plain, gap_ruled)
    started = clip.seed_mask(deg).reshape(-1, 4).all(axis=1)
    ends = ruled.status[last, 0].reshape(-1, 4).all(axis=1)
    assert (ends & ~started).any(), "no tag that started hidden ends tracked"
    assert (ruled.rec[:, 0, H.ST_NVISIBLE] * 4 == ruled.status[:, 0].sum(axis=1)).all()


# --------------------------------------------------------------------------------------------------- composition and refusals
def _cap_run(seq, prelude=None, view_deg=0.0):
    """6 frames of the camera-facing cap (seq640) under reproject -> (records, final status)"""
    import torch
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    frames = torch.from_numpy(seq.frames()).cuda()
    trk = StreamTracker(seq.width, seq.height, seq.obj, seq.K, None, n_streams=1, reproject=True, view_deg=view_deg)
    if prelude is not None:
        prelude(trk)
    trk.reset(frames[0:1].contiguous(), torch.from_numpy(seq.corners(0)[None]).cuda().contiguous())
    so = trk.new_state_buffer(len(seq) - 1)
    for k in range(1, len(seq)):
        trk.step(frames[k:k + 1], so[k - 1])
    trk.join()
    torch.cuda.synchronize()
    st = np.zeros((1, seq.obj.shape[0]), np.uint8)
    H.check(trk.ctx.L.agt_download(trk.ctx.h, st.ctypes.data_as(C.c_void_p), C.c_void_p(trk.corners()[1]), st.nbytes), "agt_download")
    return so.cpu().numpy(), st


def test_off_is_off_and_90_degrees_on_the_cap_changes_only_the_count(torch_cuda, seq640):
    from accurate_aprilgroup_tracking_amd import hiplib as H

    def on_then_off(trk):
        trk.visibility(70.0)
        trk.visibility(0.0)
    never, st0 = _cap_run(seq640)
    off, st1 = _cap_run(seq640, prelude=on_then_off)
    assert (never[:, 0, H.ST_OK] == 1).all() and (never[:, 0, H.ST_NVISIBLE] == 0).all()
    assert np.array_equal(never.view(np.uint64), off.view(np.uint64)), "rule switched off: records differ from a tracker that never had it"
    assert np.array_equal(st0, st1) and st0.all()
    at90, st2 = _cap_run(seq640, view_deg=90.0)
    assert (at90[:, 0, H.ST_NVISIBLE] == 12).all() and st2.all()
    rest = [i for i in range(H.STATE_STRIDE) if i != H.ST_NVISIBLE]
    assert np.array_equal(at90[:, :, rest].view(np.uint64), never[:, :, rest].view(np.uint64)), "every tag of the cap is visible: same records"


def test_dense_frames_are_refused_while_the_rule_is_on(torch_cuda, seq640):
    import torch
    from accurate_aprilgroup_tracking_amd import hiplib as H, synthetic as syn
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = seq640
    mx = syn.model_samples(s.group, 8)
    T = np.nan_to_num(syn.sample_bilinear(s.frame(0), syn.project(mx, s.rvecs[0], s.tvecs[0], s.K)), nan=128.0).astype(np.float32)
    trk = StreamTracker(s.width, s.height, s.obj, s.K, None, reproject=True, view_deg=70.0)
    trk.dense_model(torch.from_numpy(mx).cuda(), torch.from_numpy(T).cuda(), iters=2, photo_weight=0.05, reseed=True)
    f = [torch.from_numpy(s.frame(k)[None]).cuda().contiguous() for k in (0, 1)]
    trk.reset(f[0], torch.from_numpy(s.corners(0)[None]).cuda().contiguous())
    for call in (lambda: trk.step_dense(f[1]), lambda: trk.step_many_dense(f[1][None])):
        with pytest.raises(H.AgtError) as e:
            call()
        assert e.value.code == -6                      # AGT_ERR_UNSUPPORTED
    trk.visibility(0.0)
    so = trk.new_state_buffer()
    do = trk.step_dense(f[1], so)
    torch.cuda.synchronize()
    assert so.cpu().numpy()[0, H.ST_OK] == 1 and do.cpu().numpy()[0, H.DN_VALID] > 0, "the dense frame runs again once the rule is off"
    # the entry point's own argument checks, on a live tracker of 48 corners
    for args in ((4, -1.0, 1), (4, 90.5, 1), (4, float("nan"), 1), (4, float("inf"), 1), (4, 70.0, 0), (4, 70.0, 2), (3, 70.0, 1), (5, 70.0, 1), (0, 0.0, 1)):
        assert trk.ctx.L.agt_tracker_visibility(trk.ctx.h, *args) == -1, args
    trk.visibility(70.0, corners_per_tag=6)            # 48 = 8 x 6
    # a later reset whose corner count is no whole number of tags is refused while the rule is on
    odd = StreamTracker(s.width, s.height, s.obj[:46], s.K, None, reproject=True)
    odd.visibility(70.0)
    with pytest.raises(H.AgtError) as e:
        odd.reset()
    assert e.value.code == -1
    odd.visibility(0.0)
    odd.reset()
    # on the reset tracker of 46 corners: switching on is refused, switching off always succeeds
    assert odd.ctx.L.agt_tracker_visibility(odd.ctx.h, 4, 70.0, 1) == -1
    odd.visibility(0.0)
    # a tracker without reproject refuses the rule in visibility() as in its constructor (a silent no-op otherwise); off is accepted
    bare = StreamTracker(s.width, s.height, s.obj, s.K, None)
    with pytest.raises(ValueError, match="reproject"):
        bare.visibility(70.0)
    bare.visibility(0.0)


def test_the_rule_composes_with_the_forward_backward_check(torch_cuda, chains):
    """fb_check = 1 px on the 12-tag clips: the chain applies both rules -- a corner the check drops comes back with the refresh only
    if its tag is visible"""
    deg = S.VIEW_DEG[12]
    steps = (S.STEP_DEG, -S.STEP_DEG)
    want = [chains(12, s, deg, 1.0) for s in steps]
    for b, recs in enumerate(want):
        _assert_scene_works(recs, deg, "12 tags with the check, step %g" % steps[b])
    run = DeviceRun([S.ClosedBodyClip.get(12, s) for s in steps], deg, fb_px=1.0)
    for b, recs in enumerate(want):
        _assert_chain(run, b, recs, "12 tags at %g deg with the check" % deg)
