"""The fused step's frame chains over clips whose records go through the branches of the pose role's frame tail, held bitwise to the
serial order (depth 0, whose LK step is the general body, not the chained one) at every launch depth, cut into step_many calls and
stream count.  What this file pins today is the chained LK role (agt_lk_chain_body.h) and the unchanged frame-to-frame hand-over of the
pose role; a two-stage hand-over between the pose role's waves has to keep every one of these records (the form that publishes after
the LM loop did, and was dropped for its speed: profiles/pose_handover.md).

Clip 1 (37 frames): the start-up frames of the motion model (n_vel 0, 1, 2), a gate rejection in the middle of a launch, the next frame
solved without a guess, and accepted frames with the model running again.  The rejected frame is a SHEARED copy of a frame of the
sequence (x' = x + 0.06 (y - 240), at most 9 px at the corners' rows): LK follows the tag corners to their sheared places (the physical
points, so the next true frame brings them back), and no rigid pose explains a shear -- the mean reprojection error is 3.1 px against the
2 px gate.  A frame of another scene or a blank one is rejected too, but the raw corner chain never recovers from it (the corners stay
where the foreign texture took them, or are lost for good), so the "solved without a guess" and "model runs again" frames would not
follow.

Clip 2 (13 frames) holds a BLANK frame instead: it is rejected with every corner still tracked, the frame after it loses every corner
(nothing to differentiate in a blank previous image) and, a lost corner staying lost, every later frame ends on the too-few-points path
before the solve -- frames that end without a pose, in the middle of a launch and at its end.

640 x 480, three pyramid levels: the smallest frame the chained role is tested at in this project, all three levels still hold whole tiles."""
import json
import logging
import os

import numpy as np
import pytest

SHEAR = 0.06
BAD = 7                                      # index of the sheared frame in the clip
N = 37                                       # prime: no depth of the tests divides the clip, every run ends on a drain
BASE = [1, 2, 3, 4, 5, 4, 3, 2, 1, 0]
ORDER = [BASE[i % len(BASE)] for i in range(N)]
DEPTHS = (0, 1, 2, 3, 5, 32)


def sheared(img):
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    h, w = img.shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    uv = np.stack([xx - SHEAR * (yy - h / 2.0), yy], -1).reshape(-1, 2)
    v = np.nan_to_num(syn.sample_bilinear(img.astype(np.float64), uv), nan=0.0).reshape(h, w)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def clip_frames(seq640):
    """[N, H, W] uint8: the clip, the sheared frame at BAD"""
    fr = [seq640.frame(k) for k in ORDER]
    fr[BAD] = sheared(fr[BAD])
    return np.stack(fr)


def assert_cases(ok, ntrack, guess, tvec_f32):
    """the per-frame facts (arrays over the clip) show every case the clip was built for; a condition of the tests, not a measurement"""
    assert ok[0] and not guess[0], "first frame: solved without a guess"
    assert guess[1] and not tvec_f32[1], "n_vel 0: solved from the previous solve's pose"
    assert guess[2] and not tvec_f32[2], "n_vel 1: the model has one velocity, the guess is still the pose"
    assert tvec_f32[3], "n_vel 2: the model's guess (float32 tvec) is in use"
    assert 0 < BAD < min(d for d in DEPTHS if d > BAD) - 1, "the rejected frame is inside a launch"
    assert not ok[BAD] and ntrack[BAD] == 48 and guess[BAD], "gate rejection with every corner tracked"
    assert ok[BAD + 1] and not guess[BAD + 1] and ntrack[BAD + 1] == 48, "the next frame is solved without a guess"
    assert ok[BAD + 2] and guess[BAD + 2] and not tvec_f32[BAD + 2], "then from that pose"
    assert tvec_f32[BAD + 3:].all() and guess[BAD + 3:].all(), "and the model runs again"
    assert ok[np.arange(N) != BAD].all()


def test_oracle_chain_shows_every_case(oracle, seq640, clip_frames):
    """CPU: the oracle chain (oracle LK + the PoseDetector mirror, as test_fused_track_frame_matches_oracle_chain drives it) over the
    clip goes through every case -- the scenario is a property of the clip, not of the device code"""
    import tempfile
    from oracle import cv2_shim
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    s = seq640
    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "april_group.json"), "w").write(json.dumps(s.group))

    class Det(PoseDetector):
        DIRPATH = tmp
    det = Det(logging.getLogger("test_gpu_pose_handover"), s.K, s.dist, True, cv=cv2_shim.make_cv2())
    obj32 = s.obj.astype(np.float32)
    pts = s.corners(0)
    pyr = oracle.Pyramid(s.frame(0))
    ok, ntrack, guess, f32 = [np.zeros(N, bool) for _ in range(4)]
    ntrack = np.zeros(N, int)
    for i in range(N):
        npyr = oracle.Pyramid(clip_frames[i])
        nx, status, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, maxLevel=2)
        nx = nx.reshape(-1, 2); status = status.ravel()
        g = det.extrinsic_guess
        guess[i] = g[0] is not None
        f32[i] = guess[i] and g[1].dtype == np.float32
        il = [nx[j].reshape(1, 1, 2) for j in range(48) if status[j]]
        ol = [obj32[j].reshape(1, 3) for j in range(48) if status[j]]
        det._estimate_pose(il if len(il) >= 8 else [], ol if len(il) >= 8 else [])
        ntrack[i] = int(status.sum())
        ok[i] = det.last_error is not None and det.last_error < 2
        if i == BAD:
            assert det.last_error > 2.5, "the rejection is not marginal: %g" % det.last_error
        pts = nx.astype(np.float32)
        pyr = npyr
    assert_cases(ok, ntrack, guess, f32)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


def state_bytes(st):
    return bytes(st)[:-4]                    # (all fields but the struct's trailing pad word)


def run(torch, s, clip, depth, B=1, cuts=None, join_at_cuts=False):
    """clip [n, B, H, W] -> records [n, B, STATE_STRIDE], [state bytes per stream]; cuts None: one step() per frame, else step_many over clip[a:b]"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=B)
    trk.pipeline(depth)
    f0 = torch.from_numpy(s.frame(0)).cuda().unsqueeze(0).expand(B, -1, -1).contiguous()
    trk.reset(f0, torch.from_numpy(np.repeat(s.corners(0)[None], B, 0)).cuda().contiguous())
    n = clip.shape[0]
    so = torch.zeros((n, B, H.STATE_STRIDE), dtype=torch.float64, device="cuda")
    if cuts is None:
        for i in range(n):
            trk.step(clip[i], so[i])
    else:
        assert cuts[0] == 0 and cuts[-1] == n
        for a, b in zip(cuts[:-1], cuts[1:]):
            trk.step_many(clip[a:b], so[a:b])
            if join_at_cuts:
                trk.join()
    trk.join()
    states = trk.read_state()
    assert all(st.frame == n for st in states)
    return so.cpu().numpy(), [state_bytes(st) for st in states]


def device_clip(torch, clip_frames, B):
    return torch.from_numpy(clip_frames).cuda().unsqueeze(1).expand(-1, B, -1, -1).contiguous()        # [N, B, H, W]


@pytest.fixture(scope="module")
def serial(torch_cuda, seq640, clip_frames):
    """records and state of the serial order (depth 0, one stream), with the cases asserted"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    rec, st = run(torch_cuda, seq640, device_clip(torch_cuda, clip_frames, 1), 0)
    r = rec[:, 0]
    assert not (r[:, H.ST_FLAGS].astype(int) & H.TRK_CHAIN_TIMEOUT).any()
    assert_cases(r[:, H.ST_OK] == 1, r[:, H.ST_NTRACK].astype(int), r[:, H.ST_GUESS] == 1, r[:, H.ST_TVEC_F32] == 1)
    assert r[BAD, H.ST_ERR] > 2.5
    return rec, st


@pytest.mark.gpu
def test_records_and_state_bitwise_across_depths(torch_cuda, seq640, clip_frames, serial):
    """one step() per frame at every depth: launches of 1, 2, 3, 5 and 32 frames, each run ending on a drain (37 frames)"""
    clip = device_clip(torch_cuda, clip_frames, 1)
    for depth in DEPTHS[1:]:
        rec, st = run(torch_cuda, seq640, clip, depth)
        assert np.array_equal(rec.view(np.uint64), serial[0].view(np.uint64)), "depth %d" % depth
        assert st == serial[1], "depth %d" % depth


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 2, 3, 5, 32])
def test_clips_that_do_not_fill_their_launches(torch_cuda, seq640, clip_frames, serial, depth):
    """step_many over pieces of 7, 1, 15 and 14 frames and over the whole clip; with a join after every piece each piece ends on a
    drain of its own, so launches of odd and of even frame counts occur (the last frame's state write-back lands on either wave)"""
    clip = device_clip(torch_cuda, clip_frames, 1)
    for cuts, join_at_cuts in (((0, 7, 8, 23, N), False), ((0, 7, 8, 23, N), True), ((0, N), False)):
        rec, st = run(torch_cuda, seq640, clip, depth, cuts=cuts, join_at_cuts=join_at_cuts)
        assert np.array_equal(rec.view(np.uint64), serial[0].view(np.uint64)), "depth %d cuts %s join %s" % (depth, cuts, join_at_cuts)
        assert st == serial[1], "depth %d cuts %s join %s" % (depth, cuts, join_at_cuts)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 5, 32])
def test_three_streams_equal_the_one_stream_run(torch_cuda, seq640, clip_frames, serial, depth):
    """B = 3 (144 corners: still the fused form): every stream's records and state are those of the one-stream serial run"""
    clip = device_clip(torch_cuda, clip_frames, 3)
    rec, st = run(torch_cuda, seq640, clip, depth, B=3, cuts=(0, 7, 8, 23, N))
    for b in range(3):
        assert np.array_equal(rec[:, b].view(np.uint64), serial[0][:, 0].view(np.uint64)), "stream %d" % b
        assert st[b] == serial[1][0], "stream %d" % b


# ---- clip 2: a blank frame, then too few points
N2 = 13
BAD2 = 6


@pytest.fixture(scope="module")
def blank_clip_frames(seq640):
    fr = [seq640.frame(k) for k in ORDER[:N2]]
    fr[BAD2] = np.zeros_like(fr[BAD2])
    return np.stack(fr)


def test_oracle_blank_frame_is_rejected_and_loses_every_corner(oracle, seq640, blank_clip_frames):
    """CPU: oracle LK over the blank frame keeps every corner (status 1) at places no pose explains, and finds no corner in the frame
    after it.  (The oracle's LK has no memory of a lost corner; the tracker's status is sticky, so its later frames stay without points.)"""
    s = seq640
    pts = s.corners(0)
    pyr = oracle.Pyramid(s.frame(0))
    for i in range(BAD2 + 2):
        npyr = oracle.Pyramid(blank_clip_frames[i])
        nx, status, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, maxLevel=2)
        n = int(status.sum())
        assert n == (0 if i == BAD2 + 1 else 48), "frame %d: %d corners" % (i, n)
        if i == BAD2:
            truth = s.corners(ORDER[i])
            assert np.abs(nx.reshape(-1, 2) - truth).max() > 20, "the blank frame leaves the corners where a pose could explain them"
        pts = nx.reshape(-1, 2).astype(np.float32)
        pyr = npyr


@pytest.mark.gpu
def test_blank_frame_then_too_few_points_bitwise_across_depths(torch_cuda, seq640, blank_clip_frames):
    """frames that end before the solve (too few points), after a rejected one, inside launches of every depth and at their ends"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    clip = device_clip(torch_cuda, blank_clip_frames, 1)
    ref, ref_st = run(torch_cuda, seq640, clip, 0)
    r = ref[:, 0]
    assert (r[:BAD2, H.ST_OK] == 1).all()
    assert r[BAD2, H.ST_OK] == 0 and r[BAD2, H.ST_NTRACK] == 48 and r[BAD2, H.ST_GUESS] == 1 and r[BAD2, H.ST_ERR] > 2.5, "gate rejection"
    assert (r[BAD2 + 1:, H.ST_OK] == 0).all() and (r[BAD2 + 1:, H.ST_NTRACK] == 0).all(), "every corner lost, and lost for good"
    assert (r[BAD2 + 1:, H.ST_ITERS] == 0).all() and (r[BAD2 + 1:, H.ST_FLAGS] != 0).all(), "no solve: the too-few-points record"
    assert not (r[:, H.ST_FLAGS].astype(int) & H.TRK_CHAIN_TIMEOUT).any()
    for depth in DEPTHS[1:]:
        for cuts in (None, (0, 4, 9, N2)):
            rec, st = run(torch_cuda, seq640, clip, depth, cuts=cuts, join_at_cuts=cuts is not None)
            assert np.array_equal(rec.view(np.uint64), ref.view(np.uint64)), "depth %d cuts %s" % (depth, cuts)
            assert st == ref_st, "depth %d cuts %s" % (depth, cuts)
