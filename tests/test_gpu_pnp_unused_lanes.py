"""-m gpu: a lane WITHOUT a correspondence contributes exactly nothing to a pose solve.

The per-lane sums of an LM evaluation (csrc/agt_pnp_body.h evaluate_t: the 28 of a Jacobian pass, |e|^2, the epilogue's error sum)
start from the lane's first point instead of from a zero the point is added to; a lane that holds no point -- beyond n, or masked
out -- hands zeros to the wave sum that are written elsewhere.  If such a lane ever contributed what it computed, or what its
registers happened to hold, these tests show it: every masked case runs twice, the second time with the image points of the masked
corners set to NaN and their object points to 1e30, and pose, info and error of the two runs must be the same bits.  Each run is
also held to the oracle's solvePnP on the unmasked subset (POSE_TOL = 1e-9 on identical inputs, equal iteration counts).

Sizes: n = 4, 5, 47, 48, 63, 64 run the one-point-per-lane kernel (pnp_kernel<T, 1>); n = 65 and 240 with a guess run the four
cooperating waves (one point per lane each: at 65 two waves hold no point at all), and WITHOUT a guess the four-points-per-lane body
(DLT start; the suite's bound for guess-less solves is 1e-8, tests/test_gpu_parity.py).  Masks: none; every third tag (four
consecutive corners) off -- holes in the middle of the wave; only the last four corners left.  Cameras: pinhole and MILD_DIST.
The same through StreamTracker.step at depth 1 and 3: a 160 x 120 clip of five frames, two tags lost at the first frame."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pnp_numpy                       # noqa: E402

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-9          # pose against the oracle on identical inputs (tests/test_gpu_parity.py)
NOGUESS_TOL = 1e-8       # ... of a solve without a guess (tests/test_gpu_parity.py, tests/test_gpu_pose_range.py)
SIZES_ONE_WAVE = (4, 5, 47, 48, 63, 64)
SIZES_BIG = (65, 240)
TRUTH = np.array([0.31, -0.22, 0.17, 0.012, -0.021, 0.42])
GUESS = TRUTH + np.array([0.02, -0.015, 0.01, 0.002, 0.003, -0.01])


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    from accurate_aprilgroup_tracking_amd import cv_hip
    return cv_hip.Context(64, 64, max_level=0, max_points=256, max_streams=8)


def camera(distorted):
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    return syn.camera_matrix(640, 480), (syn.MILD_DIST if distorted else None)


def scene(n, K, dist):
    """n generic points in a 10 cm box, their projections under TRUTH with 0.05 px of noise"""
    rng = np.random.default_rng(1000 + n)
    obj = rng.uniform(-0.05, 0.05, (n, 3))
    img = pnp_numpy.project(obj, TRUTH[:3], TRUTH[3:], K, dist) + rng.normal(0, 0.05, (n, 2))
    return obj, img


def masks(n, with_last_four=True):
    """-> [(name, mask (n,) u8 | None)]"""
    i = np.arange(n)
    out = [("none", None), ("every third tag off", ((i // 4) % 3 != 1).astype(np.uint8))]
    if with_last_four:
        out.append(("last four only", (i >= n - 4).astype(np.uint8)))
    return out


def run_cases(torch, ctx, oracle, n, distorted, use_guess, tol):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    K, dist = camera(distorted)
    obj, img = scene(n, K, dist)
    cases = masks(n, with_last_four=use_guess)          # (a solve without a guess needs six points)
    # streams: the unmasked case once, every masked case clean and poisoned
    rows = []
    for name, m in cases:
        rows.append((name, m, False))
        if m is not None:
            rows.append((name, m, True))
    B = len(rows)
    objs, imgs, mk = np.tile(obj, (B, 1, 1)), np.tile(img, (B, 1, 1)), np.ones((B, n), np.uint8)
    for b, (name, m, poisoned) in enumerate(rows):
        if m is not None:
            mk[b] = m
            if poisoned:
                imgs[b, m == 0] = np.nan
                objs[b, m == 0] = 1e30
    pose = torch.from_numpy(np.tile(GUESS, (B, 1))).cuda().contiguous() if use_guess else None
    pose, info, err = ctx.solve_pnp(torch.from_numpy(objs).cuda().contiguous(), torch.from_numpy(imgs).cuda().contiguous(), K, dist,
                                    pose, use_guess, torch.from_numpy(mk).cuda().contiguous())
    pose, info, err = pose.cpu().numpy(), info.cpu().numpy(), err.cpu().numpy()
    clean = {}
    for b, (name, m, poisoned) in enumerate(rows):
        where = "n %d, %s, %s, mask %s%s" % (n, "mild_dist" if distorted else "pinhole", "guess" if use_guess else "no guess", name,
                                           ", poisoned" if poisoned else "")
        if poisoned:
            a = clean[name]
            same = (np.array_equal(pose[a].view(np.uint64), pose[b].view(np.uint64)) and np.array_equal(info[a], info[b])
                    and err[a:a + 1].view(np.uint64)[0] == err[b:b + 1].view(np.uint64)[0])
            print("%s: pose %s info %s err %.17g -- %s" % (where, pose[b], info[b], err[b], "same bits as the clean run" if same else "DIFFERS from the clean run"))
            assert same, where
            continue
        clean[name] = b
        sub = np.flatnonzero(m) if m is not None else np.arange(n)
        if use_guess:
            ok, r_o, t_o, it_o = oracle.solvePnP(obj[sub], img[sub], K, dist, GUESS[:3].copy(), GUESS[3:].copy(), True, return_iters=True)
        else:
            ok, r_o, t_o, it_o = oracle.solvePnP(obj[sub], img[sub], K, dist, return_iters=True)
        d = np.abs(pose[b] - np.concatenate([r_o.ravel(), t_o.ravel()])).max()
        print("%s: %d points used, |device - oracle| = %.3g (bound %.3g), iterations %d (oracle %d)"
              % (where, info[b, H.INFO_NUSED], d, tol, info[b, H.INFO_ITERS], it_o))
        assert info[b, H.INFO_OK] == 1 and info[b, H.INFO_NUSED] == len(sub), where
        assert np.isfinite(pose[b]).all() and np.isfinite(err[b]), where
        assert d <= tol, where
        assert info[b, H.INFO_ITERS] == it_o, where


@pytest.mark.parametrize("distorted", [False, True], ids=["pinhole", "mild_dist"])
@pytest.mark.parametrize("n", SIZES_ONE_WAVE + SIZES_BIG)
def test_solve_with_a_guess(torch_cuda, ctx, oracle, n, distorted):
    run_cases(torch_cuda, ctx, oracle, n, distorted, True, POSE_TOL)


@pytest.mark.parametrize("distorted", [False, True], ids=["pinhole", "mild_dist"])
@pytest.mark.parametrize("n", SIZES_BIG)
def test_four_points_per_lane_without_a_guess(torch_cuda, ctx, oracle, n, distorted):
    run_cases(torch_cuda, ctx, oracle, n, distorted, False, NOGUESS_TOL)


# ------------------------------------------------------------------------------------------------------------- through the tracker
LOST_TAGS = (3, 8)


@pytest.fixture(scope="module")
def clip():
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    seq = syn.Sequence(160, 120, n_tags=12, n_frames=6, seed=0, supersample=2)
    return seq, seq.frames()


@pytest.mark.parametrize("depth", [1, 3])
def test_tracker_records_do_not_see_lost_corners(torch_cuda, clip, depth):
    """two tags start outside the image, so LK loses them at the first frame (status 0, position carried) and the pose role masks
    them in all five frames; in the second run their start positions are NaN (a wild position: lost up front, agt_lk_body.h
    lk_pt_ok) and their object points 1e30.  The five records are the same bits."""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    seq, frames = clip
    fr = torch.from_numpy(frames).cuda()
    lost = np.zeros(4 * 12, bool)
    for t in LOST_TAGS:
        lost[4 * t:4 * t + 4] = True
    records = []
    for poisoned in (False, True):
        obj = seq.obj.astype(np.float32).copy()
        start = seq.corners(0).copy()
        start[lost] = np.nan if poisoned else -500.0
        if poisoned:
            obj[lost] = 1e30
        trk = StreamTracker(160, 120, obj, seq.K, None, n_streams=1)
        trk.pipeline(depth)
        trk.reset(fr[0:1].contiguous(), torch.from_numpy(start[None]).cuda().contiguous())
        so = trk.new_state_buffer(5)
        so = so.view(5, 1, H.STATE_STRIDE)
        for k in range(5):
            trk.step(fr[k + 1:k + 2].contiguous(), so[k])
        trk.join()
        torch.cuda.synchronize()
        records.append(so.cpu().numpy()[:, 0])
    a, b = records
    for k in range(5):
        print("depth %d frame %d: ok %d, corners used %d, err %.6g px, iterations %d, flags %d | poisoned: ok %d, used %d, err %.6g"
              % (depth, k + 1, a[k, H.ST_OK], a[k, H.ST_NTRACK], a[k, H.ST_ERR], a[k, H.ST_ITERS], a[k, H.ST_FLAGS],
                 b[k, H.ST_OK], b[k, H.ST_NTRACK], b[k, H.ST_ERR]))
    assert (a[:, H.ST_NTRACK] == 48 - 4 * len(LOST_TAGS)).all(), "the two tags are lost, the other ten tracked"
    assert (a[:, H.ST_OK] == 1).all() and np.isfinite(a).all() and (a[1:, H.ST_GUESS] == 1).all()
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), "records differ"
