"""-m gpu: the device rotation and projection code (csrc/agt_device.h: agt_rodrigues, agt_sincos, agt_project, agt_rodrigues_inv)
over the whole range of rotations, through the entry points that expose it, against the EXACT statement of the operations
(tests/pose_exact.py, mpmath; tabulated in tests/golden/pose_range.npz -- this module reads only the table).

The rest of the suite runs at |rvec| ~ 0.4 and compares with float64 statements whose own Jacobian cancels at small angles
(tests/test_pose_exact.py prints by how much), under a bound of 1e-7.  Here every branch point of those functions is crossed --
theta = 0 and below DBL_EPSILON (identity select), the series below 1e-2 and the closed form from 1e-2 on, every quadrant of the
hand-written sincos and its library fall-back at 2^20, theta = pi from both sides; the zero rule, the theta = pi branch with its sign
fix-ups and the scaled branch of the matrix-to-vector code, its Newton-Schulz and its SVD side -- under bounds that come from rounding:

  pixels, f64      |device - exact| <= 128 eps max(|u|, |v|, fx)
  Jacobian         per point, rotation 2 x 3 block and translation 2 x 3 block apart: 128 eps * the block's largest |exact entry|
                   (some 40 rounded operations lie between rvec and an entry of the 14-coefficient path, each within an ulp of a
                   quantity of the block's scale; the translation columns, f / Z = 2250, would hide the rotation block's G, 20 times
                   smaller, under a common scale)
  theta > 2 pi     both bounds times theta: half an ulp of the angle itself moves the result by that much
  pixels, f32      the exact pixel of the float32-valued inputs rounded to float32, within one float32 ulp
  pose_pred        exactly zero under the zero rule; the oracle's Rodrigues(matrix) within POSE_TOL = 1e-9 in the theta = pi branch
                   (signs included); elsewhere R(pose_pred) against the exact rotation entrywise within 128 eps, |pose_pred| <= pi;
                   the translation within 128 eps max|t|
  solvePnP         noise-free recovery within 1e-8, iteration counts and poses as the oracle's where the oracle's Jacobian is exact;
                   without a guess, device against oracle within 1e-8
  state machine    tests/test_gpu_tracker.py's comparison and bound (1e-8), through R = I and through theta = pi

Every figure is printed before it is asserted; profiles/pose_range.md records them.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pnp_numpy                       # noqa: E402
import pose_range_scenes as prs        # noqa: E402
from pose_range_scenes import block_ratios, pixel_ratios      # noqa: E402

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
RND = 128 * EPS
POSE_TOL = 1e-9          # pose against the oracle on identical inputs
RECOVERY_TOL = 1e-8      # noise-free recovery (test_gpu_parity.py::test_full_size_properties_without_the_oracle); planar init; state machine
CAMS = ("pinhole", "mild", "tilt14")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


@pytest.fixture(scope="module")
def table():
    return dict(np.load(os.path.join(HERE, "golden", "pose_range.npz")))


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    from accurate_aprilgroup_tracking_amd import cv_hip
    return cv_hip.Context(64, 64, max_level=0, max_points=64, max_streams=64)


def dist_of(table, cam):
    return None if cam == "pinhole" else table["dist_" + cam]


def angle_factor(theta):
    return np.where(theta > 2 * np.pi, theta, 1.0)


def report(what, ratio, bound):
    """ratio, bound: arrays of one shape, first axis = rung; prints the largest ratio to its bound and where, then asserts"""
    q = ratio / bound
    i = np.unravel_index(np.argmax(q), q.shape)
    print("%s: largest ratio to its bound %.3g (%.3g eps against %.3g eps) at rung %d"
          % (what, q[i], ratio[i] / EPS, np.broadcast_to(bound, q.shape)[i] / EPS, i[0]))
    assert (q <= 1.0).all(), what


# ------------------------------------------------------------------------------------------- projection and Jacobian over the ladder
def check_projection(table, cam, px, J):
    """px (B, 6, 2), J (B, 12, 6) | None from the device: the f64 bounds of the module docstring"""
    f = angle_factor(table["theta"])[:, None]
    report("%s pixels" % cam, pixel_ratios(px, table["px_" + cam]), RND * f)
    if J is not None:
        r = block_ratios(J.reshape(-1, 6, 2, 6), table["jac_" + cam])
        report("%s rotation block" % cam, r[..., 0], RND * f)
        report("%s translation block" % cam, r[..., 1], RND * f)


def check_projection_f32(table, cam, px):
    want = table["px32_" + cam].astype(np.float32)
    ulps = np.abs(px.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
    i = np.unravel_index(np.argmax(ulps), ulps.shape)
    print("%s float32 pixels: off by at most %.3g ulp (rung %d)" % (cam, ulps[i], i[0]))
    assert px.dtype == np.float32 and (ulps <= 1.0).all()


@pytest.mark.parametrize("cam", CAMS)
def test_projection_and_jacobian_over_the_ladder(torch_cuda, ctx, table, cam):
    torch = torch_cuda
    obj = torch.from_numpy(table["obj"]).cuda().contiguous()
    pose = torch.from_numpy(table["pose"]).cuda().contiguous()
    K, dist = table["K"], dist_of(table, cam)
    px, J = ctx.project_points(obj, pose, K, dist, jacobian=True)
    check_projection(table, cam, px.cpu().numpy(), J.cpu().numpy())
    # the other template instance
    px, J = ctx.project_points(obj, pose, K, dist, jacobian=False)
    assert J is None
    check_projection(table, cam, px.cpu().numpy(), None)
    # float32 object points
    obj32 = torch.from_numpy(table["obj"].astype(np.float32)).cuda().contiguous()
    for jac in (True, False):
        px, J = ctx.project_points(obj32, pose, K, dist, jacobian=jac)
        check_projection_f32(table, cam, px.cpu().numpy())


@pytest.mark.parametrize("cam", CAMS)
def test_points_in_and_behind_the_camera_plane(torch_cuda, ctx, table, cam):
    """z = 0 exactly (the kernel's `z != 0 ? rcp : 1`) and z < 0: the device equals the plain formula"""
    torch = torch_cuda
    K, dist = table["K"], dist_of(table, cam)
    t = table["pose"][0, 3:]
    obj = np.array([[0.003, -0.002, -t[2]], [0.01, 0.01, -t[2] - 0.1], [-0.02, 0.015, -t[2] - 0.3], [0.01, -0.01, 0.0]])
    poses = np.array([np.concatenate([np.zeros(3), t]), np.concatenate([1e-17 * prs.AXIS, t])])
    assert (obj @ np.eye(3) + t)[0, 2] == 0.0 and ((obj + t)[1:3, 2] < 0).all()
    for jac in (True, False):
        px, _ = ctx.project_points(torch.from_numpy(obj).cuda(), torch.from_numpy(poses).cuda(), K, dist, jacobian=jac)
        px = px.cpu().numpy()
        want = np.stack([pnp_numpy.project(obj, p[:3], p[3:], K, dist) for p in poses])
        assert np.isfinite(want).all()
        report("%s z = 0, z < 0 (jacobian=%s)" % (cam, jac), pixel_ratios(px, want), RND)


# --------------------------------------------------------------------------- agt_rodrigues_inv through agt_predict_flow's pose_pred
def check_pose_pred(table, oracle, pred):
    kind, Rp, tp = table["inv_kind"], table["inv_Rp"], table["inv_tp"]
    assert pred.shape == (len(kind), 6) and np.isfinite(pred).all()
    pis, gen = np.flatnonzero(kind == 1), np.flatnonzero(kind == 2)
    want = {m: oracle.Rodrigues(Rp[m])[0].ravel() for m in pis}
    d_pi = np.array([np.abs(pred[m, :3] - want[m]).max() for m in pis])
    dR = np.array([np.abs(pnp_numpy.rodrigues(pred[m, :3])[0] - Rp[m]).max() for m in gen])
    dt = np.abs(pred[:, 3:] - tp).max(axis=1) / np.abs(tp).max()
    for m, d in zip(pis, d_pi):
        print("pi rung %2d: |device - oracle| = %.3g   device %s" % (m, d, pred[m, :3]))
    for m, d in zip(gen, dR):
        print("generic rung %2d: |R(pose_pred) - exact| = %.3g eps   device %s" % (m, d / EPS, pred[m, :3]))
    print("translation: %.3g eps of max|t|; theta = pi branch against the oracle: %.3g (bound %.3g)" % (dt.max() / EPS, d_pi.max(), POSE_TOL))
    for m in np.flatnonzero(kind == 0):
        assert not pred[m, :3].any(), "rung %d: the zero rule" % m
    assert (d_pi <= POSE_TOL).all(), "theta = pi branch"
    for m in pis:
        big = np.abs(want[m]) > POSE_TOL
        assert np.array_equal(np.sign(pred[m, :3][big]), np.sign(want[m][big])), "rung %d: signs" % m
    assert (dR <= RND).all(), "generic rungs"
    assert (np.linalg.norm(pred[gen, :3], axis=1) <= np.pi).all()
    assert (dt <= RND).all(), "translation"


def test_matrix_to_vector_through_predict_flow(torch_cuda, ctx, table, oracle):
    """older = (0, t2), newer = (phi / 2 * a, t1): the predicted rotation is exp(phi a), pose_pred its agt_rodrigues_inv; 26 rungs,
    one launch.  With OpenCV's theta = acos(c) and the axis from the antisymmetric part alone the generic rungs at phi = 2e-5,
    pi - 1e-3, pi - 2e-5 and pi + 1e-3 read 2.4e3, 629, 1.4e4 and 691 eps against the bound of 128; agt_rodrigues_inv was changed for
    it (asin below sin = 1/4, the symmetric part beyond a quarter turn) and reads 0.03, 1, 1 and 3.5 eps (profiles/pose_range.md)."""
    torch = torch_cuda
    h = 0.01
    obj = np.array([[-h, -h, 0], [-h, h, 0], [h, h, 0], [h, -h, 0.0]])
    B = len(table["inv_kind"])
    prev = np.zeros((B, 4, 2), np.float32)
    out = ctx.predict_flow(torch.from_numpy(obj).cuda(), torch.from_numpy(table["inv_older"]).cuda().contiguous(),
                           torch.from_numpy(table["inv_newer"]).cuda().contiguous(), table["K"], None, torch.from_numpy(prev).cuda(), None, 1e9)
    torch.cuda.synchronize()
    check_pose_pred(table, oracle, out[3].cpu().numpy())


# ------------------------------------------------------------------------------------------------------------- solvePnP at the rungs
@pytest.mark.parametrize("cam", ["pinhole", "mild"])
def test_solve_pnp_with_a_guess_at_the_rungs(torch_cuda, ctx, table, oracle, cam):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    obj, truth, guess, img = table["pnp_obj"], table["pnp_truth"], table["pnp_guess"], table["pnp_img_" + cam]
    K, dist = table["K"], dist_of(table, cam)
    theta = np.linalg.norm(truth[:, :3], axis=1)
    pose = torch.from_numpy(guess.copy()).cuda()
    pose, info, _ = ctx.solve_pnp(torch.from_numpy(obj).cuda(), torch.from_numpy(img).cuda().contiguous(), K, dist, pose, True)
    pose, info = pose.cpu().numpy(), info.cpu().numpy()
    for q in range(len(truth)):
        ok, r_o, t_o, it_o = oracle.solvePnP(obj, img[q], K, dist, guess[q, :3].copy(), guess[q, 3:].copy(), True, return_iters=True)
        d_o = np.abs(pose[q] - np.concatenate([r_o.ravel(), t_o.ravel()])).max()
        print("%s theta %.17g: |device - truth| %.3g, |device - oracle| %.3g, iterations %d (oracle %d)"
              % (cam, theta[q], np.abs(pose[q] - truth[q]).max(), d_o, info[q, H.INFO_ITERS], it_o))
    for q in range(len(truth)):
        assert info[q, H.INFO_OK] == 1
        assert np.abs(pose[q] - truth[q]).max() <= RECOVERY_TOL, "theta %.17g" % theta[q]
        if theta[q] == 0.0 or theta[q] >= 5e-3:
            ok, r_o, t_o, it_o = oracle.solvePnP(obj, img[q], K, dist, guess[q, :3].copy(), guess[q, 3:].copy(), True, return_iters=True)
            assert info[q, H.INFO_ITERS] == it_o, "theta %.17g" % theta[q]
            assert np.abs(pose[q] - np.concatenate([r_o.ravel(), t_o.ravel()])).max() <= POSE_TOL, "theta %.17g" % theta[q]


PLANAR_TURNS = {"identity": np.zeros(3), "pi about x": np.array([np.pi, 0.0, 0.0]), "pi - 5e-6": (np.pi - 5e-6) * prs.AXIS, "1e-3": 1e-3 * prs.AXIS}


def planar_cases():
    """-> [(name, obj (n, 3))]: one frontal 20 mm tag; ten coplanar points"""
    h = 0.01
    rng = np.random.default_rng(6)
    return [("tag", np.array([[-h, -h, 0], [-h, h, 0], [h, h, 0], [h, -h, 0.0]])),
            ("ten points", np.concatenate([rng.uniform(-0.05, 0.05, (10, 2)), np.zeros((10, 1))], axis=1))]


@pytest.mark.parametrize("distorted", [False, True], ids=["pinhole", "mild_dist"])
def test_solve_pnp_without_a_guess_frontal_and_half_turn(torch_cuda, ctx, table, oracle, distorted):
    """homography -> agt_rodrigues_inv (SVD side) -> agt_rodrigues -> the LM from rvec = 0 (R = I exactly) or from the half turn"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import synthetic as syn, hiplib as H
    K = syn.camera_matrix(640, 480)
    dist = syn.MILD_DIST if distorted else None
    t = np.array([0.01, 0.02, 0.4])
    rng = np.random.default_rng(60)
    for name, obj in planar_cases():
        img = np.stack([pnp_numpy.project(obj, r, t, K, dist) + rng.normal(0, 0.02, (len(obj), 2)) for r in PLANAR_TURNS.values()])
        pose, info, _ = ctx.solve_pnp(torch.from_numpy(obj).cuda(), torch.from_numpy(img).cuda().contiguous(), K, dist)
        pose, info = pose.cpu().numpy(), info.cpu().numpy()
        worst = 0.0
        for q, turn in enumerate(PLANAR_TURNS):
            ok, r_o, t_o = oracle.solvePnP(obj, img[q], K, dist)
            d = np.abs(pose[q] - np.concatenate([r_o.ravel(), t_o.ravel()])).max()
            print("%s, %s, %s: |device - oracle| = %.3g   device %s" % (name, turn, "mild_dist" if distorted else "pinhole", d, pose[q]))
            assert info[q, H.INFO_OK] == 1 and info[q, H.INFO_FLAGS] & H.PNP_PLANAR
            worst = max(worst, d)
        assert worst <= RECOVERY_TOL, name


# ------------------------------------------------------------------------------------- the state machine through R = I and theta = pi
@pytest.mark.parametrize("variant", ["identity", "pi"])
def test_state_machine_through(torch_cuda, oracle, variant):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    sc = prs.TurnScene(variant)
    ref = prs.mirror_run(sc)
    assert ref["pose_valid"].all() and prs.guess_sign_changes(ref) == 1
    B = 2
    trk = StreamTracker(1280, 720, ref["all_objpts"], sc.K, sc.dist, n_streams=B, enhance_ape=True)
    trk.reset()
    so = trk.new_state_buffer()
    mask = torch.ones((B, 4 * prs.N_TAGS), dtype=torch.uint8, device="cuda")
    worst = 0.0
    for k in range(prs.N_FRAMES):
        img = torch.from_numpy(np.repeat(sc.corners[k][None].astype(np.float32), B, 0)).cuda().contiguous()
        trk.estimate_pose(img, mask, so)
        st = so.cpu().numpy()
        states = trk.read_state()
        for b in range(B):
            assert int(st[b, H.ST_OK]) == ref["pose_valid"][k] == 1, "frame %d acceptance" % k
            d = [np.abs(st[b, :6] - ref["pose"][k]).max()]
            s = states[b]
            assert s.has_guess == ref["guess_valid"][k], "frame %d guess presence" % k
            if s.has_guess:
                d.append(np.abs(np.array(s.guess[:]) - ref["guess"][k]).max())
            assert s.n_vel == ref["n_vel"][k], "frame %d velocities" % k
            for i in range(s.n_vel):
                d.append(np.abs(np.array(s.rot_vel[i][:]) - ref["rot_vel"][k][i]).max())
                d.append(np.abs(np.array(s.tran_vel[i][:]) - ref["tran_vel"][k][i]).max())
            assert s.has_prev and ref["prev_valid"][k]
            d.append(np.abs(np.array(s.prev[:]) - ref["prev"][k]).max())
            if b == 0:
                print("%s frame %2d: pose, guess, velocities, previous pose differ by at most %.3g   guess %s" % (variant, k, max(d), np.array(s.guess[:3])))
            assert max(d) < RECOVERY_TOL, "frame %d stream %d: %s" % (k, b, d)
            worst = max(worst, max(d))
    print("%s: largest difference %.3g (bound %.3g)" % (variant, worst, RECOVERY_TOL))
