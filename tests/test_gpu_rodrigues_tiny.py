"""-m gpu: agt_rodrigues (csrc/agt_device.h) at and below theta = DBL_EPSILON, where it returns R = I.

The case is taken on the INPUTS of the entries (the unit axis is forced to zero; cos = 1, 1 - cos = 0 and the series values 1/2, 1/6
come out of the general code there by themselves), not by selects on the 18 results.  R is the identity exactly; the derivative G is
the identity only to ~|r| / 2 off the diagonal -- which is its true value.  Four rotation vectors (0; 1e-17 e_x; 3e-16 (1, 1, 1) /
sqrt 3, above DBL_EPSILON: the general path right beside the case; 1e-12 e_z), six points, the three cameras of the pose ladder,
through project_points with the Jacobian, against the exact statement (tests/pose_exact.py, tabulated in
tests/golden/rodrigues_tiny.npz by tests/golden/make_rodrigues_tiny_fixture.py) under the bounds of tests/test_gpu_pose_range.py:
128 eps of max(|u|, |v|, fx) on the pixels, 128 eps of the block's largest exact entry on the rotation and translation blocks.
R = I exactly: with rvec = 0 and operands chosen so that every operation of the pinhole formula is exact in float64 (dyadic points,
1 / z a power of two), the pixels equal the plain formula's bit for bit.  And a solve that STARTS at rvec = 0 (its first evaluation
takes the case, with the Jacobian) agrees with the oracle to 1e-9 with the same number of iterations."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pnp_numpy                       # noqa: E402
from pose_range_scenes import block_ratios, pixel_ratios      # noqa: E402

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
RND = 128 * EPS          # tests/test_gpu_pose_range.py
POSE_TOL = 1e-9
CAMS = ("pinhole", "mild", "tilt14")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


@pytest.fixture(scope="module")
def table():
    return dict(np.load(os.path.join(HERE, "golden", "rodrigues_tiny.npz")))


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    from accurate_aprilgroup_tracking_amd import cv_hip
    return cv_hip.Context(64, 64, max_level=0, max_points=64, max_streams=8)


def test_table_holds_the_four_rotations(table):
    th = table["theta"]
    assert th[0] == 0.0 and th[1] == 1e-17 and th[1] < EPS < th[2] < 4e-16 and th[3] == 1e-12
    assert np.array_equal(table["rvec"][1], [1e-17, 0, 0]) and np.array_equal(table["rvec"][3], [0, 0, 1e-12])
    assert np.ptp(table["rvec"][2]) == 0.0 and table["obj"].shape == (4, 6, 3)


@pytest.mark.parametrize("cam", CAMS)
def test_projection_and_jacobian_at_tiny_rotations(torch_cuda, ctx, table, cam):
    torch = torch_cuda
    obj = torch.from_numpy(table["obj"]).cuda().contiguous()
    pose = torch.from_numpy(table["pose"]).cuda().contiguous()
    dist = None if cam == "pinhole" else table["dist_" + cam]
    for jac in (True, False):
        px, J = ctx.project_points(obj, pose, table["K"], dist, jacobian=jac)
        px = px.cpu().numpy()
        r = pixel_ratios(px, table["px_" + cam])
        print("%s pixels (jacobian=%s): %s eps per rotation (bound 128)" % (cam, jac, np.round(r.max(axis=1) / EPS, 3)))
        assert (r <= RND).all(), "%s pixels" % cam
        if jac:
            b = block_ratios(J.cpu().numpy().reshape(-1, 6, 2, 6), table["jac_" + cam])
            print("%s rotation block: %s eps per rotation; translation block: %s eps (bound 128)"
                  % (cam, np.round(b[..., 0].max(axis=1) / EPS, 3), np.round(b[..., 1].max(axis=1) / EPS, 3)))
            assert (b[..., 0] <= RND).all(), "%s rotation block" % cam
            assert (b[..., 1] <= RND).all(), "%s translation block" % cam


def test_pixels_at_zero_rotation_equal_the_plain_formula(torch_cuda, ctx, table):
    """z = 1/2, 1/4, 1/8 and x, y multiples of 2^-10: (X + tx) / z, its product with f = 900 and the sum with the principal point are
    exact in float64, so is the device's reciprocal (a power of two survives the Newton steps) -- any R but the exact identity with
    a visible effect, and any rounding, would show"""
    torch = torch_cuda
    K = table["K"]
    t = np.array([3.0 / 1024, -5.0 / 1024, 0.375])
    obj = np.array([[-10, -10, 128], [-10, 10, 128], [10, 10, 128], [10, -10, 128], [0, 0, -128], [37, -21, -256]], np.float64) / 1024.0
    z = obj[:, 2] + t[2]
    assert set(z) <= {0.5, 0.25, 0.125}
    want = np.stack([(obj[:, 0] + t[0]) / z * K[0, 0] + K[0, 2], (obj[:, 1] + t[1]) / z * K[1, 1] + K[1, 2]], axis=1)
    assert np.array_equal(want, pnp_numpy.project(obj, np.zeros(3), t, K, None))
    poses = np.array([np.concatenate([np.zeros(3), t]), np.concatenate([[1e-17, 0, 0], t])])
    for jac in (True, False):
        px, _ = ctx.project_points(torch.from_numpy(obj).cuda(), torch.from_numpy(poses).cuda(), K, None, jacobian=jac)
        px = px.cpu().numpy()
        print("rvec = 0 and 1e-17 e_x (jacobian=%s): largest |device - plain formula| = %g" % (jac, np.abs(px - want).max()))
        assert np.array_equal(px[0], want) and np.array_equal(px[1], want)


@pytest.mark.parametrize("distorted", [False, True], ids=["pinhole", "mild_dist"])
def test_solve_started_at_zero_rotation(torch_cuda, ctx, oracle, distorted):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import synthetic as syn, hiplib as H
    K = syn.camera_matrix(640, 480)
    dist = syn.MILD_DIST if distorted else None
    rng = np.random.default_rng(12)
    obj = rng.uniform(-0.05, 0.05, (12, 3))
    truth = np.array([0.06, -0.045, 0.03, 0.01, -0.02, 0.4])
    img = pnp_numpy.project(obj, truth[:3], truth[3:], K, dist)          # noise-free
    guess = np.array([0.0, 0.0, 0.0, 0.012, -0.018, 0.41])
    pose = torch.from_numpy(guess[None].copy()).cuda()
    pose, info, _ = ctx.solve_pnp(torch.from_numpy(obj).cuda(), torch.from_numpy(img[None]).cuda().contiguous(), K, dist, pose, True)
    pose, info = pose.cpu().numpy()[0], info.cpu().numpy()[0]
    ok, r_o, t_o, it_o = oracle.solvePnP(obj, img, K, dist, guess[:3].copy(), guess[3:].copy(), True, return_iters=True)
    d = np.abs(pose - np.concatenate([r_o.ravel(), t_o.ravel()])).max()
    print("start at rvec = 0: |device - oracle| = %.3g (bound %.3g), |device - truth| = %.3g, iterations %d (oracle %d)"
          % (d, POSE_TOL, np.abs(pose - truth).max(), info[H.INFO_ITERS], it_o))
    assert info[H.INFO_OK] == 1 and d <= POSE_TOL and info[H.INFO_ITERS] == it_o
