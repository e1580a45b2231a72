"""-m gpu: tag-consensus PnP, the stateless call (agt_solve_pnp_consensus) -- bitwise against the composition of the library's own
agt_solve_pnp / agt_project_points calls, and against the CPU oracle's composition of the rule (tests/consensus_scenes.py, whose
batches test_tag_consensus.py holds to the margin condition on the CPU)."""
import ctypes as C

import numpy as np
import pytest

import consensus_scenes as S

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-9            # the project's PnP tolerance (tests/test_gpu_parity.py)
SENTINEL = 7.0


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    from accurate_aprilgroup_tracking_amd import cv_hip
    return cv_hip.Context(64, 64, max_level=0, win=21, max_points=256, max_streams=8)


_BATCH = {}


def batch(kind, oracle):
    if kind not in _BATCH:
        _BATCH[kind] = S.make_batch(kind, oracle)
    return _BATCH[kind]


def device_run(torch, ctx, bt, dtype, guess):
    """the consensus call -> host arrays"""
    td = torch.float32 if dtype == "f32" else torch.float64
    obj = torch.from_numpy(bt.obj).cuda().to(td).contiguous()
    img = torch.from_numpy(bt.img).cuda().to(td).contiguous()
    mask = None if bt.mask is None else torch.from_numpy(bt.mask).cuda().contiguous()
    pose0 = bt.guess.copy() if guess else np.full((bt.B, 6), SENTINEL)
    pose = torch.from_numpy(pose0).cuda().contiguous()
    out = ctx.solve_pnp_consensus(obj, img, bt.K, bt.dist, pose, guess, mask, 4, S.TAU, S.MIN_INLIERS)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out), (obj, img, mask, pose0)


def composed(torch, ctx, bt, dev, guess):
    """the same result from agt_solve_pnp on the reshaped arrays, numpy votes on agt_project_points' f64 output, agt_solve_pnp on the
    elected mask"""
    obj, img, mask, pose0 = dev
    B, n, T = bt.B, bt.n, bt.n // 4
    hobj = obj.reshape(1, T, 4, 3).expand(B, T, 4, 3).reshape(B * T, 4, 3).contiguous()
    himg = img.reshape(B * T, 4, 2).contiguous()
    hmask = None if mask is None else mask.reshape(B * T, 4).contiguous()
    hpose = torch.from_numpy(np.repeat(pose0, T, axis=0)).cuda().contiguous()
    hpose, hinfo, _ = ctx.solve_pnp(hobj, himg, bt.K, bt.dist, hpose, guess, hmask)
    proj, _ = ctx.project_points(obj.double().contiguous(), hpose, bt.K, bt.dist)
    torch.cuda.synchronize()
    hpose_h, hinfo_h, proj_h = hpose.cpu().numpy(), hinfo.cpu().numpy(), proj.cpu().numpy()
    from accurate_aprilgroup_tracking_amd import hiplib as H
    img_h = img.cpu().numpy()
    inl = np.zeros((B, n), np.uint8); votes = np.zeros((B, 4), np.int32); start = pose0.copy()
    for b in range(B):
        rows = [hpose_h[b * T + t].copy() for t in range(T)]
        tag_of = {id(r): t for t, r in enumerate(rows)}
        res = S.rule(bt.obj, img_h[b], bt.usable(b), lambda t: (rows[t], int(hinfo_h[b * T + t, H.INFO_FLAGS])),
                     lambda p: proj_h[b * T + tag_of[id(p)]])
        inl[b] = res["inliers"]
        votes[b] = (res["winner"], res["count"], res["n_cand"], res["n_hyp"])
        if res["winner"] >= 0:
            start[b] = res["pose"]
    pose = torch.from_numpy(start).cuda().contiguous()
    pose, info, err = ctx.solve_pnp(obj, img, bt.K, bt.dist, pose, True, torch.from_numpy(inl).cuda().contiguous())
    torch.cuda.synchronize()
    return pose.cpu().numpy(), inl, votes, info.cpu().numpy(), err.cpu().numpy()


CASES = [("b3_n48", "f32"), ("b3_n48", "f64"), ("b3_n48_masked", "f32"), ("b2_n240", "f32"), ("b2_n240", "f64"), ("b1_n8", "f32"),
         ("b1_n8", "f64"), ("b2_allbad", "f32"), ("b1_tilt", "f64")]


@pytest.mark.parametrize("guess", [False, True], ids=["no_guess", "guess"])
@pytest.mark.parametrize("kind,dtype", CASES)
def test_consensus_call_against_its_composition_and_the_oracle(torch_cuda, ctx, oracle, kind, dtype, guess):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    bt = batch(kind, oracle)
    (pose, inl, votes, info, err), dev = device_run(torch_cuda, ctx, bt, dtype, guess)
    # (a) bitwise: the library's own calls, composed
    c_pose, c_inl, c_votes, c_info, c_err = composed(torch_cuda, ctx, bt, dev, guess)
    assert np.array_equal(inl, c_inl), "inlier bytes differ at %s" % (np.argwhere(inl != c_inl)[:8].tolist(),)
    assert np.array_equal(votes, c_votes), "votes %s, composed %s" % (votes.tolist(), c_votes.tolist())
    assert np.array_equal(pose.view(np.uint64), c_pose.view(np.uint64)), "pose differs by %g" % np.abs(pose - c_pose).max()
    assert np.array_equal(info, c_info) and np.array_equal(err.view(np.uint64), c_err.view(np.uint64))
    # (b) the oracle's composition of the rule
    for b in range(bt.B):
        res = S.oracle_rule(oracle, bt.obj, bt.img[b], bt.K, bt.dist, usable=bt.usable(b), guess=bt.guess[b] if guess else None)
        where = "%s %s stream %d" % (kind, dtype, b)
        assert np.array_equal(inl[b].astype(bool), res["inliers"]), where + ": inlier set"
        assert np.array_equal(inl[b].astype(bool), bt.expected[b]), where + ": not the undisplaced corners"
        assert votes[b].tolist() == [res["winner"], res["count"], res["n_cand"], res["n_hyp"]], where
        ref = S.oracle_refit(oracle, bt.obj, bt.img[b], bt.K, bt.dist, res)
        if ref is None:
            # no consensus: bytes all 0, pose untouched, info OK = 0 with TOO_FEW
            start = bt.guess[b] if guess else np.full(6, SENTINEL)
            assert not inl[b].any() and np.array_equal(pose[b], start), where
            assert info[b, H.INFO_OK] == 0 and info[b, H.INFO_FLAGS] == H.PNP_TOO_FEW and votes[b, 0] == -1 and err[b] == 0.0
            continue
        assert info[b, H.INFO_OK] == 1 and info[b, H.INFO_NUSED] == res["count"]
        d = np.abs(pose[b] - ref[0]).max()
        print("%s: |hip - oracle| = %.2e, LM iterations %d / %d, winner %d with %d inliers" % (where, d, info[b, H.INFO_ITERS], ref[1], votes[b, 0], votes[b, 1]))
        assert d <= POSE_TOL, where + ": pose differs from the oracle's by %g" % d
        assert info[b, H.INFO_ITERS] == ref[1], where + ": LM iterations %d, oracle %d" % (info[b, H.INFO_ITERS], ref[1])
    if kind == "b2_allbad":
        assert votes[1].tolist() == [-1, 0, 12, 12] and votes[0, 0] >= 0


def test_batched_object_arrays_and_null_votes(torch_cuda, ctx, oracle):
    """[B][n][3] object points (a stride instead of the shared array) give the shared array's result; d_votes may be NULL"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    torch = torch_cuda
    bt = batch("b3_n48", oracle)
    (pose, inl, votes, info, err), (obj, img, mask, pose0) = device_run(torch, ctx, bt, "f32", True)
    objB = obj.reshape(1, bt.n, 3).expand(bt.B, bt.n, 3).contiguous()
    p2 = torch.from_numpy(pose0).cuda().contiguous()
    pose2, inl2, votes2, info2, err2 = ctx.solve_pnp_consensus(objB, img, bt.K, bt.dist, p2, True, None, 4, S.TAU, S.MIN_INLIERS)
    torch.cuda.synchronize()
    assert np.array_equal(pose2.cpu().numpy().view(np.uint64), pose.view(np.uint64)) and np.array_equal(inl2.cpu().numpy(), inl)
    assert np.array_equal(votes2.cpu().numpy(), votes) and np.array_equal(info2.cpu().numpy(), info)
    p3 = torch.from_numpy(pose0).cuda().contiguous()
    inl3 = torch.zeros((bt.B, bt.n), dtype=torch.uint8, device="cuda")
    Kh = np.ascontiguousarray(bt.K, np.float64); dh = np.ascontiguousarray(bt.dist, np.float64).ravel()
    rc = ctx.L.agt_solve_pnp_consensus(ctx.h, C.c_void_p(obj.data_ptr()), 0, C.c_void_p(img.data_ptr()), H.F32, None, bt.n, bt.B,
                                       Kh.ctypes.data_as(C.c_void_p), dh.ctypes.data_as(C.c_void_p), dh.size, C.c_void_p(p3.data_ptr()), 1,
                                       4, S.TAU, S.MIN_INLIERS, C.c_void_p(inl3.data_ptr()), None, None, None)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(inl3.cpu().numpy(), inl) and np.array_equal(p3.cpu().numpy().view(np.uint64), pose.view(np.uint64))


def test_error_codes(torch_cuda, ctx, oracle):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    torch = torch_cuda
    bt = batch("b3_n48", oracle)
    obj = torch.from_numpy(bt.obj).cuda().contiguous(); img = torch.from_numpy(bt.img).cuda().contiguous()
    pose = torch.zeros((bt.B, 6), dtype=torch.float64, device="cuda")
    for kw, code in ((dict(inlier_px=0.0), -1), (dict(inlier_px=-2.0), -1), (dict(inlier_px=float("nan")), -1), (dict(inlier_px=float("inf")), -1),
                     (dict(corners_per_tag=3), -1), (dict(corners_per_tag=5), -1), (dict(min_inliers=3), -1)):
        with pytest.raises(H.AgtError) as e:
            ctx.solve_pnp_consensus(obj, img, bt.K, bt.dist, pose, False, None, **kw)
        assert e.value.code == code, kw
    big = torch.zeros((1, 260, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(H.AgtError) as e:
        ctx.solve_pnp_consensus(torch.zeros((260, 3), dtype=torch.float32, device="cuda"), big, bt.K, bt.dist, None, False, None)
    assert e.value.code == -4                          # AGT_ERR_NPOINTS: n > 256, 65 tags
    torch.cuda.synchronize()
    assert not pose.cpu().numpy().any(), "a refused call wrote the pose"


def test_cv_shaped_call(torch_cuda, oracle):
    """cv_hip.solvePnPTagConsensus: (ok, rvec, tvec, inliers (k,1) int32) as cv2.solvePnPRansac shapes them; the guess arrays are not written"""
    from accurate_aprilgroup_tracking_amd import cv_hip
    sc = S.Scene(12, 1, 3, group_seed=0)
    img = sc.img()
    for guess in (False, True):
        r0, t0 = sc.guess[:3].copy().reshape(3, 1), sc.guess[3:].copy().reshape(3, 1)
        ok, rvec, tvec, inliers = cv_hip.solvePnPTagConsensus(sc.obj, img, sc.K, sc.dist, r0 if guess else None, t0 if guess else None, guess)
        res = S.oracle_rule(oracle, sc.obj, img, sc.K, sc.dist, guess=sc.guess if guess else None)
        ref, _ = S.oracle_refit(oracle, sc.obj, img, sc.K, sc.dist, res)
        assert ok and inliers.dtype == np.int32 and inliers.shape == (36, 1) and rvec.shape == (3, 1) and tvec.shape == (3, 1)
        assert np.array_equal(inliers.ravel(), np.flatnonzero(sc.clean))
        assert np.abs(np.concatenate([rvec.ravel(), tvec.ravel()]) - ref).max() <= POSE_TOL
        assert np.array_equal(r0.ravel(), sc.guess[:3]) and np.array_equal(t0.ravel(), sc.guess[3:])
    bad = S.Scene(12, 1, all_bad=True, group_seed=0)
    ok, rvec, tvec, inliers = cv_hip.solvePnPTagConsensus(bad.obj, bad.img(), bad.K, bad.dist)
    assert not ok and inliers.shape == (0, 1) and not rvec.any() and not tvec.any()
