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


def device_run(torch, ctx, bt, dtype, guess, min_inliers=None):
    """the consensus call -> host arrays.  bt.obj: (n,3), shared by the streams, or (B,n,3): the [B][n][3] form, obj_batch_stride = 3n"""
    td = torch.float32 if dtype == "f32" else torch.float64
    obj = torch.from_numpy(bt.obj).cuda().to(td).contiguous()
    img = torch.from_numpy(bt.img).cuda().to(td).contiguous()
    mask = None if bt.mask is None else torch.from_numpy(bt.mask).cuda().contiguous()
    pose0 = bt.guess.copy() if guess else np.full((bt.B, 6), SENTINEL)
    pose = torch.from_numpy(pose0).cuda().contiguous()
    out = ctx.solve_pnp_consensus(obj, img, bt.K, bt.dist, pose, guess, mask, bt.cpt, S.TAU, bt.min_inliers if min_inliers is None else min_inliers)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out), (obj, img, mask, pose0)


def composed(torch, ctx, bt, dev, guess, min_inliers=None):
    """the same result from agt_solve_pnp on the reshaped arrays (T problems of cpt points per stream; cpt > 64: the four-wave kernel
    there too), numpy votes on agt_project_points' f64 output, agt_solve_pnp on the elected mask"""
    obj, img, mask, pose0 = dev
    cpt = bt.cpt
    B, n, T = bt.B, bt.n, bt.n // cpt
    shared = obj.dim() == 2
    hobj = (obj.reshape(1, T, cpt, 3).expand(B, T, cpt, 3) if shared else obj).reshape(B * T, cpt, 3).contiguous()
    himg = img.reshape(B * T, cpt, 2).contiguous()
    hmask = None if mask is None else mask.reshape(B * T, cpt).contiguous()
    hpose = torch.from_numpy(np.repeat(pose0, T, axis=0)).cuda().contiguous()
    hpose, hinfo, _ = ctx.solve_pnp(hobj, himg, bt.K, bt.dist, hpose, guess, hmask)
    pobj = obj.double().contiguous() if shared else obj.double().repeat_interleave(T, dim=0).contiguous()
    proj, _ = ctx.project_points(pobj, hpose, bt.K, bt.dist)
    torch.cuda.synchronize()
    hpose_h, hinfo_h, proj_h = hpose.cpu().numpy(), hinfo.cpu().numpy(), proj.cpu().numpy()
    from accurate_aprilgroup_tracking_amd import hiplib as H
    img_h = img.cpu().numpy()
    inl = np.zeros((B, n), np.uint8); votes = np.zeros((B, 4), np.int32); start = pose0.copy()
    for b in range(B):
        rows = [hpose_h[b * T + t].copy() for t in range(T)]
        tag_of = {id(r): t for t, r in enumerate(rows)}
        res = S.rule(bt.obj_of(b), img_h[b], bt.usable(b), lambda t: (rows[t], int(hinfo_h[b * T + t, H.INFO_FLAGS])),
                     lambda p: proj_h[b * T + tag_of[id(p)]], cpt=cpt, min_inliers=bt.min_inliers if min_inliers is None else min_inliers)
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


def check_call(torch, ctx, oracle, bt, kind, dtype, guess):
    """one consensus call held to (a) the composition of the library's own calls, bitwise, and (b) the oracle's composition of the rule;
    every stream, every corner.  -> (pose, inl, votes, info, err)"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    (pose, inl, votes, info, err), dev = device_run(torch, ctx, bt, dtype, guess)
    # (a) bitwise: the library's own calls, composed
    c_pose, c_inl, c_votes, c_info, c_err = composed(torch, ctx, bt, dev, guess)
    assert np.array_equal(inl, c_inl), "inlier bytes differ at %s" % (np.argwhere(inl != c_inl)[:8].tolist(),)
    assert np.array_equal(votes, c_votes), "votes %s, composed %s" % (votes.tolist(), c_votes.tolist())
    assert np.array_equal(pose.view(np.uint64), c_pose.view(np.uint64)), "pose differs by %g" % np.abs(pose - c_pose).max()
    assert np.array_equal(info, c_info) and np.array_equal(err.view(np.uint64), c_err.view(np.uint64))
    # (b) the oracle's composition of the rule
    for b in range(bt.B):
        res = bt.reference(oracle, b, guess)
        where = "%s %s stream %d" % (kind, dtype, b)
        assert np.array_equal(inl[b].astype(bool), res["inliers"]), where + ": inlier set"
        assert np.array_equal(inl[b].astype(bool), bt.expected[b]), where + ": not the undisplaced corners"
        assert votes[b].tolist() == [res["winner"], res["count"], res["n_cand"], res["n_hyp"]], where
        ref = S.oracle_refit(oracle, bt.obj_of(b), bt.img[b], bt.K, bt.dist, res)
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
    return pose, inl, votes, info, err


@pytest.mark.parametrize("guess", [False, True], ids=["no_guess", "guess"])
@pytest.mark.parametrize("kind,dtype", CASES)
def test_consensus_call_against_its_composition_and_the_oracle(torch_cuda, ctx, oracle, kind, dtype, guess):
    pose, inl, votes, info, err = check_call(torch_cuda, ctx, oracle, batch(kind, oracle), kind, dtype, guess)
    if kind == "b2_allbad":
        assert votes[1].tolist() == [-1, 0, 12, 12] and votes[0, 0] >= 0


@pytest.mark.parametrize("guess", [False, True], ids=["no_guess", "guess"])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("kind", S.EDGE_BATCHES)
def test_edge_batches_against_the_composition_and_the_oracle(torch_cuda, ctx, oracle, kind, dtype, guess):
    """The edge batches of tests/consensus_scenes.py (one clause of the rule or one bound of vote_stream's arrays each; the CPU suite
    holds them to the oracle's table and shows that the outcome hangs on the clause), the same three checks as above on every stream
    and corner, then what the scene was built for.  e_flag's reference is told what the zero tag reports (the oracle sets no flag).
    Measured on the MI355X (f32 and f64 arrays give the same figures: the points are float32 values), largest |device - oracle| of the
    refit pose without / with the guess, LM iterations device = oracle: e_nonfinite 1.3e-13 / 2.5e-16, 4; e_noncoplanar 1.6e-12 / 1.4e-16, 4;
    e_tie 5.9e-16 / 8.1e-12, 1; e_behind 1.5e-16 / 1.7e-16, 4; e_t64 and e_t64_last 2.8e-17 / 5.6e-17, 3; e_t1 1.2e-12 / 1.1e-12, 1;
    e_cpt8 1.3e-16 / 3.1e-16, 3; e_cpt80 8.3e-17 / 5.6e-17, 3; e_cpt128 8.3e-17 / 5.6e-17, 3; e_flag 6.0e-11 / 6.2e-11, 4.  The zero tag of
    e_flag alone reports info [1, 1, 4, SINGULAR] and the guess with a guess, [0, 0, 4, TOO_FEW] without."""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    torch = torch_cuda
    bt = batch(kind, oracle)
    pose, inl, votes, info, err = check_call(torch, ctx, oracle, bt, kind, dtype, guess)
    if kind == "e_tie":
        assert votes[0].tolist() == [5, 8, 12, 12]
        # one more inlier asked for than the tie has: no consensus
        (p9, i9, v9, f9, e9), dev = device_run(torch, ctx, bt, dtype, guess, min_inliers=9)
        c9 = composed(torch, ctx, bt, dev, guess, min_inliers=9)
        start = bt.guess[0] if guess else np.full(6, SENTINEL)
        assert not i9.any() and np.array_equal(p9[0], start) and v9[0].tolist() == [-1, 0, 12, 12]
        assert f9[0].tolist() == [0, 0, 0, H.PNP_TOO_FEW] and e9[0] == 0.0
        assert np.array_equal(c9[1], i9) and np.array_equal(c9[2], v9) and np.array_equal(c9[0].view(np.uint64), p9.view(np.uint64))
    if kind == "e_t64_last":
        # the winner sits in the last slot of the kernel's arrays; elected set and pose follow the permutation of e_t64
        (p0, i0, v0, f0, e0), _ = device_run(torch, ctx, batch("e_t64", oracle), dtype, guess)
        a, z = slice(4 * S.E_T64_WINNER, 4 * S.E_T64_WINNER + 4), slice(252, 256)
        perm = i0.copy(); perm[0, a], perm[0, z] = i0[0, z], i0[0, a]
        assert votes[0, 0] == 63 and v0[0, 0] == S.E_T64_WINNER and votes[0, 1:].tolist() == v0[0, 1:].tolist()
        assert np.array_equal(inl, perm) and np.abs(pose - p0).max() <= POSE_TOL and f0[0, H.INFO_ITERS] == info[0, H.INFO_ITERS]
    if kind == "e_behind":
        twins = np.flatnonzero(bt.mask[0] == 0) // 4
        assert twins.size == 2 and not any(inl[0, 4 * d + 1:4 * d + 4].any() for d in twins), "a corner behind the camera was elected"
    if kind == "e_nonfinite":
        bad = np.flatnonzero(~np.isfinite(bt.img[0]).all(axis=1))
        assert bad.size == 2 and not inl[0, bad].any() and np.isfinite(pose).all() and np.isfinite(err).all()
    if kind == "e_flag":
        # what the zero tag's own solve reports (printed; without a guess the reason it is no hypothesis is not asserted)
        t, (obj, img, mask, pose0) = S.E_FLAG_TAG, device_run(torch, ctx, bt, dtype, guess)[1]
        p1 = torch.from_numpy(pose0.copy()).cuda().contiguous()
        p1, f1, e1 = ctx.solve_pnp(obj[4 * t:4 * t + 4].contiguous(), img[:, 4 * t:4 * t + 4].contiguous(), bt.K, bt.dist, p1, guess)
        torch.cuda.synchronize()
        p1, f1 = p1.cpu().numpy()[0], f1.cpu().numpy()[0]
        print("e_flag %s %s: the zero tag alone reports info %s, pose %s" % (dtype, "guess" if guess else "no guess", f1.tolist(), p1.tolist()))
        assert votes[0, 3] == votes[0, 2] - 1 and votes[0, 0] != t
        if guess:
            assert f1[H.INFO_FLAGS] & H.PNP_SINGULAR and np.array_equal(p1, bt.guess[0]), "a finite hypothesis that only its flag disqualifies"


def test_edge_streams_in_one_call_do_not_leak_into_each_other(torch_cuda, ctx, oracle):
    """e_tie, e_behind and e_nonfinite as the three streams of one call in the [B][n][3] object form: hypotheses of one stream (discarded
    ones, a tie, a masked tag) must not be seen in the next one's LDS slots.  Bitwise the three one-stream calls."""
    torch = torch_cuda
    parts = [batch(k, oracle) for k in ("e_tie", "e_behind", "e_nonfinite")]
    st = S.StackedBatch(parts)
    for dtype in ("f32", "f64"):
        for guess in (False, True):
            pose, inl, votes, info, err = check_call(torch, ctx, oracle, st, "stacked", dtype, guess)
            for b, p in enumerate(parts):
                (p1, i1, v1, f1, e1), _ = device_run(torch, ctx, p, dtype, guess)
                where = "stream %d %s %s" % (b, dtype, guess)
                assert np.array_equal(inl[b], i1[0]) and np.array_equal(votes[b], v1[0]) and np.array_equal(info[b], f1[0]), where
                assert np.array_equal(pose[b].view(np.uint64), p1[0].view(np.uint64)) and err[b:b + 1].view(np.uint64)[0] == e1.view(np.uint64)[0], where


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
