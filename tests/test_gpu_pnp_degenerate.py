"""-m gpu: what the pose solve reports when it cannot solve -- AGT_PNP_SINGULAR, and non-finite numbers that are USED (not masked out).

The stateless agt_solve_pnp in batches of five: problem 2 is the degenerate one, the other four are healthy and must come out the same
bits as in the same call with a healthy problem 2 (one workgroup per problem: a neighbour's NaN stays its own).  n = 4 and 48 run the
one-wave body, 240 with a guess the four cooperating waves and without one the four-points-per-lane body; float32 and float64 arrays.

* Singular by construction (include/agt_hip.h AGT_PNP_SINGULAR; DESIGN.md "Deliberate, documented deviations", 2): every object point at the origin.
  The rotation columns of the Jacobian are exact zeros, the first pivot of the damped system is 0 (1 + lambda), which is not > 0: the
  step is zeroed and the flag set.  The pose is the guess, bit for bit, after one iteration; the error is the guess's.
* One used image coordinate NaN, or one used image point (+inf, +inf): J^T J does not see the image points, so the first step solves, on
  a right-hand side that is not finite; from the second step on the pivots are NaN ("not > 0"), the step is zeroed, and since no
  comparison with a NaN holds the LM loop runs to its 20 iterations.  Six pose numbers and an error that are not finite, INFO_OK = 1,
  INFO_ITERS = 20, AGT_PNP_SINGULAR (with AGT_PNP_PLANAR where the points are planar and there was no guess): the values the header
  states.  Nothing comes back finite and wrong.
* A NaN in the guess: that pose number stays NaN, same info.
* Through the tracker's state machine (StreamTracker.estimate_pose, enhance_ape on): a frame with one NaN corner is rejected
  (`esum < gate` is false for a NaN), the guess is dropped, and from the next frame on the stream's records are the same bits as after a
  frame the gate rejected with finite numbers.  No NaN survives in the state the machine reads.

Every loop on these paths is counted or capped (planarity SVD: 30 sweeps; inverse iteration: 12; undistortion: 5; homography polish: 10;
LM: 20 iterations, and its inner retry is left as soon as `errNorm > prevErrNorm` is false, which it is for a NaN).

Measured on the MI355X: singular -- info [1, 1, n, 1], error against the oracle at the guess 0 (n = 4, 48) and 2.8e-14 (n = 240); NaN / inf
image point -- six NaN, info [1, 20, n, 1] ([1, 20, 4, 3] for the planar four points without a guess); NaN guess -- that number NaN, the other
five the guess's, info [1, 20, n, 1].  Tracker: the NaN frame is record (ok 0, err NaN, 20 iterations, flags 1), the shoved one (ok 0,
err 70.0 px, 11 iterations, flags 0); frames 3 and 4 the same bits in both (err 1.02e-5 / 1.05e-5 px, 1 / 4 iterations)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pnp_numpy                       # noqa: E402

pytestmark = pytest.mark.gpu
ERR_TOL = 1e-9           # the project's bound for FP64 results on identical inputs (tests/test_gpu_parity.py)
SIZES = (4, 48, 240)
B, BAD = 5, 2
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


def camera():
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    return syn.camera_matrix(640, 480), syn.MILD_DIST


def problems(n):
    """B + 1 healthy problems (the last one is the stand-in for problem BAD): n points of a 10 cm box -- of its z = 0 face for n = 4, which
    has no start without a guess otherwise -- under TRUTH, 0.05 px of noise, float32-representable.  -> obj (B+1,n,3), img (B+1,n,2) f64"""
    K, dist = camera()
    rng = np.random.default_rng(500 + n)
    obj = rng.uniform(-0.05, 0.05, (B + 1, n, 3))
    if n == 4:
        obj[:, :, 2] = 0.0
    obj = obj.astype(np.float32).astype(np.float64)
    img = np.stack([pnp_numpy.project(obj[b], TRUTH[:3], TRUTH[3:], K, dist) for b in range(B + 1)]) + rng.normal(0, 0.05, (B + 1, n, 2))
    return obj, img.astype(np.float32).astype(np.float64)


def run(torch, ctx, obj, img, dtype, guess):
    """guess: (B,6) or None -> pose, info, err (host)"""
    K, dist = camera()
    td = torch.float32 if dtype == "f32" else torch.float64
    pose = None if guess is None else torch.from_numpy(np.ascontiguousarray(guess, np.float64)).cuda().contiguous()
    pose, info, err = ctx.solve_pnp(torch.from_numpy(obj).cuda().to(td).contiguous(), torch.from_numpy(img).cuda().to(td).contiguous(), K, dist,
                                    pose, guess is not None)
    torch.cuda.synchronize()
    return pose.cpu().numpy(), info.cpu().numpy(), err.cpu().numpy()


def with_healthy_neighbours(torch, ctx, n, dtype, guess, spoil):
    """the batch with problem BAD spoiled by spoil(obj, img, guess) (in place, problem BAD's arrays), and the same batch with the stand-in
    there: the four healthy problems must be the same bits.  -> pose, info, err, (obj, img, guess) of the spoiled run"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    obj6, img6 = problems(n)
    g = None if not guess else np.tile(GUESS, (B, 1))
    clean_obj, clean_img = obj6[:B].copy(), img6[:B].copy()
    clean_obj[BAD], clean_img[BAD] = obj6[B], img6[B]
    ref = run(torch, ctx, clean_obj, clean_img, dtype, g)
    obj, img = obj6[:B].copy(), img6[:B].copy()
    spoil(obj[BAD], img[BAD], None if g is None else g[BAD])
    out = run(torch, ctx, obj, img, dtype, g)
    keep = [b for b in range(B) if b != BAD]
    assert (ref[1][:, H.INFO_OK] == 1).all() and np.isfinite(ref[0]).all() and np.isfinite(ref[2]).all(), "the healthy batch"
    assert not (ref[1][:, H.INFO_FLAGS] & (H.PNP_SINGULAR | H.PNP_TOO_FEW)).any()
    for a, b_ in zip(ref, out):
        assert np.array_equal(np.ascontiguousarray(a[keep]).view(np.uint8), np.ascontiguousarray(b_[keep]).view(np.uint8)), \
            "a healthy problem changed beside the degenerate one"
    return out + ((obj, img, g),)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_singular_by_construction(torch_cuda, ctx, oracle, n, dtype):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    K, dist = camera()

    def spoil(obj, img, guess):
        obj[:] = 0.0
    pose, info, err, (obj, img, g) = with_healthy_neighbours(torch_cuda, ctx, n, dtype, True, spoil)
    want = oracle.mean_reproj_error(obj[BAD], img[BAD], GUESS[:3], GUESS[3:], K, dist)
    print("n %d %s: info %s, err %.12g (oracle at the guess %.12g, diff %.2e)" % (n, dtype, info[BAD].tolist(), err[BAD], want, abs(err[BAD] - want)))
    assert info[BAD, H.INFO_FLAGS] & H.PNP_SINGULAR, "a zero pivot did not set AGT_PNP_SINGULAR"
    assert np.array_equal(pose[BAD].view(np.uint64), GUESS.view(np.uint64)), "the zeroed step moved the pose"
    assert info[BAD, H.INFO_ITERS] == 1 and info[BAD, H.INFO_OK] == 1 and info[BAD, H.INFO_NUSED] == n
    assert abs(err[BAD] - want) <= ERR_TOL


@pytest.mark.parametrize("guess", [False, True], ids=["no_guess", "guess"])
@pytest.mark.parametrize("what", ["nan", "inf"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_non_finite_image_point_that_is_used(torch_cuda, ctx, n, dtype, what, guess):
    from accurate_aprilgroup_tracking_amd import hiplib as H

    def spoil(obj, img, g):
        if what == "nan":
            img[n // 2, 1] = np.nan
        else:
            img[n // 2] = np.inf
    pose, info, err, _ = with_healthy_neighbours(torch_cuda, ctx, n, dtype, guess, spoil)
    print("n %d %s %s %s: pose %s info %s err %s" % (n, dtype, what, "guess" if guess else "no guess", pose[BAD].tolist(), info[BAD].tolist(), err[BAD]))
    assert not np.isfinite(pose[BAD]).any() and not np.isfinite(err[BAD]), "a number came back finite from a solve that saw %s" % what
    planar = H.PNP_PLANAR if (n == 4 and not guess) else 0
    assert info[BAD].tolist() == [1, 20, n, H.PNP_SINGULAR | planar]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_nan_in_the_guess(torch_cuda, ctx, n, dtype):
    from accurate_aprilgroup_tracking_amd import hiplib as H

    def spoil(obj, img, g):
        g[1] = np.nan
    pose, info, err, _ = with_healthy_neighbours(torch_cuda, ctx, n, dtype, True, spoil)
    print("n %d %s: pose %s info %s err %s" % (n, dtype, pose[BAD].tolist(), info[BAD].tolist(), err[BAD]))
    assert np.isnan(pose[BAD, 1]) and not np.isfinite(err[BAD])
    assert info[BAD].tolist() == [1, 20, n, H.PNP_SINGULAR]


# ------------------------------------------------------------------------------------------------------------- through the tracker
FRAMES = 4


def tracker_run(torch, seqs, spoil):
    """four detector-fed frames of two streams -> (records (FRAMES, 2, STATE_STRIDE), [TrackState, TrackState]); spoil(corners (48,2)) edits
    frame 2 of stream 0"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    trk = StreamTracker(640, 480, seqs[0].obj.astype(np.float32), seqs[0].K, None, n_streams=2, enhance_ape=True)
    trk.reset()
    so = trk.new_state_buffer(FRAMES)
    for k in range(FRAMES):
        c = np.stack([s.corners(k) for s in seqs]).astype(np.float32)
        if k == 1 and spoil is not None:
            spoil(c[0])
        trk.estimate_pose(torch.from_numpy(c).cuda().contiguous(), None, so[k])
    torch.cuda.synchronize()
    return so.cpu().numpy(), trk.read_state()


def test_a_nan_corner_does_not_outlive_its_frame_in_the_tracker(torch_cuda):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    seqs = [syn.Sequence(640, 480, n_tags=12, n_frames=FRAMES, seed=s, group_seed=0) for s in (0, 1)]

    def nan_corner(c):
        c[17, 0] = np.nan

    def shoved(c):
        c += np.random.default_rng(7).choice(np.float32([-50.0, 50.0]), c.shape)
    clean, _ = tracker_run(torch_cuda, seqs, None)
    a, sa = tracker_run(torch_cuda, seqs, nan_corner)
    b, sb = tracker_run(torch_cuda, seqs, shoved)
    for name, r in (("clean", clean), ("A (NaN corner)", a), ("B (+-50 px)", b)):
        for k in range(FRAMES):
            print("%s frame %d stream 0: ok %g err %.6g guess %g iters %g flags %g" % (name, k + 1, r[k, 0, H.ST_OK], r[k, 0, H.ST_ERR], r[k, 0, H.ST_GUESS],
                                                                                    r[k, 0, H.ST_ITERS], r[k, 0, H.ST_FLAGS]))
    assert (clean[:, :, H.ST_OK] == 1).all() and np.isfinite(clean).all() and (clean[1:, :, H.ST_GUESS] == 1).all()
    assert a[1, 0, H.ST_OK] == 0 and not np.isfinite(a[1, 0, H.ST_ERR]) and a[1, 0, H.ST_GUESS] == 1
    assert b[1, 0, H.ST_OK] == 0 and np.isfinite(b[1, 0]).all() and b[1, 0, H.ST_ERR] > 2.0 and b[1, 0, H.ST_GUESS] == 1
    # from the next frame on a NaN rejection and a finite one are the same stream
    assert np.array_equal(a[2:, 0].view(np.uint64), b[2:, 0].view(np.uint64)), "the NaN frame left something behind"
    assert a[2, 0, H.ST_GUESS] == 0 and a[2, 0, H.ST_OK] == 1 and a[3, 0, H.ST_OK] == 1 and a[3, 0, H.ST_GUESS] == 1
    assert np.array_equal(a[0, 0].view(np.uint64), clean[0, 0].view(np.uint64))
    for r in (a, b):
        assert np.array_equal(r[:, 1].view(np.uint64), clean[:, 1].view(np.uint64)), "the clean stream saw its neighbour"
    for st_a, st_b in zip(sa, sb):
        for st in (st_a, st_b):
            assert st.has_guess == 1 and st.has_prev == 1 and st.frame == FRAMES
            read = [np.array(st.guess), np.array(st.prev), np.array(st.prev_R)] + [np.array(st.rot_vel[i]) for i in range(st.n_vel)] \
                + [np.array(st.tran_vel[i]) for i in range(st.n_vel)]
            assert all(np.isfinite(x).all() for x in read), "a non-finite number in the tracker state"
        assert bytes(st_a) == bytes(st_b), "the two rejections left different states"
