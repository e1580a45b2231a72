"""GPU: the camera calibration of libagt_camcal.so (include/agt_camcal.h) against the numpy / scipy statement of the same problem
(tests/camera_calib_numpy.py), from one evaluation up to the command-line tool.  Scenes: tests/camcal_scenes.py (640 x 480, views
tilted 17-35 degrees).

Bounds.  Residuals: 1e-9 px, the project's bound for agt_project_points.  A damped step: relative to the step's norm, ten times the
floor -- the largest difference between numpy's own Schur and dense steps over the lambdas of the scene (the two sides order their
sums differently; tests/test_camera_calib.py::test_numpy_schur_step_equals_dense_step prints the same figures on the CPU).
Recovered parameters: ten times the distance between scipy's solution and the truth.  Final cost of the noisy solve: ten times the
larger of the spread of scipy's own final cost over two different starts and n_residuals * eps, the worst-case relative rounding
error of a sum of n_residuals squares.  Every figure is printed before it is asserted; profiles/camera_calib.md records them.

The rational set with k1..k6 all free is near-singular on a 9 x 6 board at 12 views (scaled condition of J 5e7 on this scene, 2e9
with the board at 55 % of the image width instead of 70 %; 2e2 and 6e3 for the other two sets): its step is tested at lambda in
{1e-3, 10} only -- at lambda = 0 a solve of its normal equations is no reference -- and it is left out of every recovery test.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import camcal_scenes as cs          # noqa: E402
import camera_calib_numpy as cn     # noqa: E402

pytestmark = pytest.mark.gpu
EPS = float(np.finfo(np.float64).eps)
LAMBDAS = (0.0, 1e-3, 10.0)
MODELS = {"coeff5": (cs.CAM5, cs.FREE5, 5, LAMBDAS), "rational8": (cs.CAM8, cs.FREE8, 8, LAMBDAS[1:]), "prism12": (cs.CAM12, cs.FREE_PRISM, 12, LAMBDAS)}


def gpu_solver(sc, free, ndist, order=None):
    from accurate_aprilgroup_tracking_amd import camcallib
    o = range(len(sc.obj)) if order is None else order
    return camcallib.CamCal([sc.obj[v] for v in o], [sc.img[v] for v in o], cn.mask_of(dict(free=sorted(free))), ndist)


def check_eval(sc, free, ndist):
    c, p = cs.perturbed_start(sc, free)
    # the views go in shuffled: the library answers in the caller's order
    order = np.random.default_rng(0).permutation(len(sc.obj))
    shuffled = sc.subset(order)
    want = cn.residuals(shuffled.problem(free), c, p[order])
    s = gpu_solver(sc, free, ndist, order)
    got, cost = s.eval(c, p[order])
    s.close()
    d = np.abs(got - want).max()
    print("residuals: |gpu - numpy| max %.3g px (largest residual %.3g px); cost %.17g vs %.17g" % (d, np.abs(want).max(), cost, 0.5 * (want * want).sum()))
    assert got.shape == want.shape and np.abs(want).max() > 0.1
    assert d <= 1e-9
    assert abs(cost - 0.5 * (want * want).sum()) <= 1e-9 * np.abs(want).sum()


def check_step(sc, free, ndist, lambdas=LAMBDAS):
    prob = sc.problem(free)
    c, p = cs.perturbed_start(sc, free)
    dense = {lam: cn.dense_step(prob, c, p, lam) for lam in lambdas}
    floor = max(cn.step_difference(cn.schur_step(prob, c, p, lam), dense[lam]) for lam in lambdas)
    s = gpu_solver(sc, free, ndist)
    worst = 0.0
    fixed = [i for i in range(16) if i not in free]
    for lam in lambdas:
        got = s.step(lam, c, p)
        d = cn.step_difference(got, dense[lam])
        print("lambda %g: |gpu - dense| / |dense| = %.3g (floor %.3g, bound %.3g)" % (lam, d, floor, 10 * floor))
        worst = max(worst, d)
        assert np.array_equal(got[0][fixed].view(np.uint64), np.zeros(len(fixed), np.uint64))          # exactly +0.0
    s.close()
    assert worst <= 10 * floor


@pytest.mark.parametrize("name", sorted(MODELS))
def test_evaluation_parity(name):
    """every coefficient of the model non-zero (the fixed ones of the thin-prism set, k4 k5 k6, too)"""
    cam, free, ndist, _ = MODELS[name]
    assert np.all(cam[:4 + ndist] != 0.0)
    check_eval(cs.parity_scene(cam), free, ndist)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_step_parity(name):
    cam, free, ndist, lambdas = MODELS[name]
    check_step(cs.parity_scene(cam), free, ndist, lambdas)


def test_smallest_system():
    """V = 3, 4 points a view, free = {fx, fy}: 24 residuals, 20 unknowns; the 14 fixed entries come back with the bits they went in with"""
    sc = cs.smallest_scene()
    check_eval(sc, [0, 1], 5)
    check_step(sc, [0, 1], 5)
    c0, p0 = cs.perturbed_start(sc, [0, 1])
    c0[9:] = [-0.0, 1e-300, 5e-324, -3e-5, 2e-5, 1e-5, -1e-5]          # fixed entries of every kind: a negative zero, a subnormal
    s = gpu_solver(sc, [0, 1], 12)
    c1, p1, rep = s.solve(c0, p0)
    s.close()
    print("smallest: %d iterations, cost %.3g -> %.3g, fx fy %.6f %.6f -> %.6f %.6f" % (rep.iterations, rep.initial_cost, rep.final_cost, c0[0], c0[1], c1[0], c1[1]))
    assert rep.accepted >= 1 and rep.final_cost < rep.initial_cost
    assert np.array_equal(c1[2:].view(np.uint64), c0[2:].view(np.uint64)) and not np.array_equal(c1[:2], c0[:2])


def test_tile_boundary():
    """views of 4, 63, 64, 65, 128 and 129 points in one problem (the accumulation walks a view in tiles of 64)"""
    sc = cs.tile_scene()
    assert [len(o) for o in sc.obj] == [4, 63, 64, 65, 128, 129]
    check_eval(sc, cs.FREE5, 5)
    check_step(sc, cs.FREE5, 5)


@pytest.mark.parametrize("cleared", cs.FREE5)
def test_fixed_entries(cleared):
    """every single-bit mask over the 5-coefficient set: the step of the cleared entry is exactly 0, the rest is numpy's step for that mask"""
    free = [i for i in cs.FREE5 if i != cleared]
    check_step(cs.parity_scene(cs.CAM5), free, 5)


def test_noise_free_recovery():
    """8 views of a 6 x 5 grid, 9 free, started from the closed form: the solve reaches scipy's solution from the same start.
    Measured on the MI355X: see profiles/camera_calib.md."""
    from accurate_aprilgroup_tracking_amd import camera_calib as cc
    sc = cs.recovery_scene()
    rms, mtx, dist, rvecs, tvecs, rep = cc.calibrate_camera(sc.obj, sc.img, sc.size)
    c_g, p_g = rep["camera"], np.concatenate([rvecs, tvecs], axis=1)
    assert abs(rep["initial_camera"][0] / sc.cam[0] - 1) < 0.05 and abs(rep["initial_camera"][1] / sc.cam[1] - 1) < 0.05
    assert not rep["initial_camera"][4:].any() and rep["free"] == ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3"]
    c_s, p_s, cost_s, rms_s = cn.solve(sc.problem(cs.FREE5), rep["initial_camera"], rep["initial_view_poses"])
    floor = max(np.abs(c_s - sc.cam).max(), np.abs(p_s - sc.poses).max())
    d = max(np.abs(c_g - c_s).max(), np.abs(p_g - p_s).max())
    print("scipy vs truth %.3g (floor; focal %.3g px), gpu vs scipy %.3g (bound %.3g; focal %.3g px), gpu vs truth %.3g; rms scipy %.3g gpu %.3g; %d iterations, %d accepted, stop: %s"
          % (floor, np.abs(c_s - sc.cam)[:2].max(), d, 10 * floor, np.abs(c_g - c_s)[:2].max(), max(np.abs(c_g - sc.cam).max(), np.abs(p_g - sc.poses).max()),
             rms_s, rms, rep["iterations"], rep["accepted"], rep["stop_reason"]))
    assert mtx.shape == (3, 3) and dist.shape == (1, 5) and np.array_equal(dist.ravel(), c_g[4:9]) and not c_g[9:].any()
    assert rep["final_cost"] < rep["initial_cost"] and rep["accepted"] >= 1
    assert d <= 10 * floor


@pytest.fixture(scope="module")
def noisy():
    """the 20-view, sigma = 0.2 px solve with its own start (and eight more views, held out), shared by the tests below"""
    from accurate_aprilgroup_tracking_amd import camera_calib as cc
    sc = cs.noisy_scene()
    cal = sc.subset(range(cs.N_CAL))
    return sc, cal, cc.calibrate_camera(cal.obj, cal.img, cal.size)


def test_noisy_solve(noisy):
    from accurate_aprilgroup_tracking_amd import camera_calib as cc, cv_hip
    sc, cal, (rms, mtx, dist, rvecs, tvecs, rep) = noisy
    prob = cal.problem(cs.FREE5)
    # the reference from the same start, and from the truth: the spread of its own final cost is the floor
    _, _, cost_ref, _ = cn.solve(prob, rep["initial_camera"], rep["initial_view_poses"])
    _, _, cost_ref2, _ = cn.solve(prob, cal.cam, cal.poses)
    n_res = 2 * rep["n_points"]
    floor = max(abs(cost_ref - cost_ref2) / cost_ref, n_res * EPS)
    d = abs(rep["final_cost"] - cost_ref) / cost_ref
    print("final cost: gpu %.17g, scipy %.17g (from the truth: %.17g); relative difference %.3g, floor %.3g, bound %.3g; %d iterations (%d accepted), rms %.4f px"
          % (rep["final_cost"], cost_ref, cost_ref2, d, floor, 10 * floor, rep["iterations"], rep["accepted"], rms))
    print("camera: %s (truth %s)" % (np.array2string(rep["camera"][:9], precision=5), np.array2string(cal.cam[:9], precision=5)))
    assert n_res == 2 * 54 * cs.N_CAL and abs(rms - np.sqrt(2 * rep["final_cost"] / rep["n_points"])) < 1e-12
    assert d <= 10 * floor
    # held-out views: solvePnP with the calibrated camera reprojects better than with the camera the solve started from
    err = {}
    for name, c in (("calibrated", rep["camera"]), ("start", rep["initial_camera"])):
        K, dc = cc.camera_from_vector(c, 5)
        e = []
        for v in range(cs.N_CAL, cs.N_CAL + cs.N_HELD):
            ok, r, t = cv_hip.solvePnP(sc.obj[v], sc.img[v], K, dc)
            proj, _ = cv_hip.projectPoints(sc.obj[v], r, t, K, dc)
            e.append(np.linalg.norm(proj.reshape(-1, 2) - sc.img[v], axis=1).mean())
        err[name] = float(np.mean(e))
    print("held-out mean reprojection error: calibrated %.4f px, start %.4f px" % (err["calibrated"], err["start"]))
    assert err["calibrated"] < err["start"]


def test_cv_shaped_entry_point(noisy):
    """cv_hip.calibrateCamera returns cv2's shapes and the solve of calibrate_camera"""
    from accurate_aprilgroup_tracking_amd import cv_hip
    sc, cal, (rms, mtx, dist, rvecs, tvecs, rep) = noisy
    rms2, mtx2, dist2, rv2, tv2 = cv_hip.calibrateCamera(cal.obj, cal.img, cal.size, None, None)
    assert rms2 == rms and np.array_equal(mtx2, mtx) and dist2.shape == (1, 5) and np.array_equal(dist2, dist)
    assert isinstance(rv2, tuple) and isinstance(tv2, tuple) and len(rv2) == len(tv2) == cs.N_CAL
    assert all(r.shape == (3, 1) and t.shape == (3, 1) for r, t in zip(rv2, tv2))
    assert np.array_equal(np.concatenate(rv2).reshape(-1, 3), rvecs) and np.array_equal(np.concatenate(tv2).reshape(-1, 3), tvecs)


def test_determinism(noisy):
    from accurate_aprilgroup_tracking_amd import camera_calib as cc
    sc, cal, (rms, mtx, dist, rvecs, tvecs, rep) = noisy
    rms2, mtx2, dist2, rvecs2, tvecs2, rep2 = cc.calibrate_camera(cal.obj, cal.img, cal.size)
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    assert np.float64(rms).view(np.uint64) == np.float64(rms2).view(np.uint64)
    for a, b in ((mtx, mtx2), (dist, dist2), (rvecs, rvecs2), (tvecs, tvecs2)):
        assert np.array_equal(bits(a), bits(b))
    assert sorted(rep2) == sorted(rep)
    for k, v in rep.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(bits(v), bits(rep2[k])), k
        elif isinstance(v, float):
            assert np.float64(v).view(np.uint64) == np.float64(rep2[k]).view(np.uint64), k
        else:
            assert v == rep2[k], k


def test_refusals():
    from accurate_aprilgroup_tracking_amd import camcallib, camera_calib as cc, cv_hip
    ok = cs.recovery_scene()
    K, dist = cc.camera_from_vector(ok.cam, 5)
    two = ok.subset([0, 1])
    with pytest.raises(camcallib.CamCalError) as e:
        cc.calibrate_camera(two.obj, two.img, two.size)
    assert e.value.code == camcallib.ERR_TOO_FEW
    front = cs.fronto_scene()
    with pytest.raises(camcallib.CamCalError) as e:
        cc.calibrate_camera(front.obj, front.img, front.size)
    assert e.value.code == camcallib.ERR_DEGENERATE
    lifted = cs.nonplanar_scene()
    with pytest.raises(camcallib.CamCalError) as e:
        cc.calibrate_camera(lifted.obj, lifted.img, lifted.size)
    assert e.value.code == camcallib.ERR_ARG
    # ... accepted with a guess (5 % off in the focal lengths), and solved
    rms, mtx, _, _, _, rep = cc.calibrate_camera(lifted.obj, lifted.img, lifted.size, K * [[1.05, 1, 1], [1, 0.95, 1], [1, 1, 1]], np.zeros(5),
                                                 flags=cv_hip.CALIB_USE_INTRINSIC_GUESS)
    print("non-planar target with a guess: rms %.3g px after %d iterations, fx %.6f fy %.6f" % (rms, rep["iterations"], mtx[0, 0], mtx[1, 1]))
    assert rms < 1e-6 and abs(mtx[0, 0] - lifted.cam[0]) < 1e-5
    with pytest.raises(camcallib.CamCalError) as e:
        gpu_solver(ok, cs.FREE5, 14)
    assert e.value.code == camcallib.ERR_CAMERA
    with pytest.raises(camcallib.CamCalError) as e:
        cc.calibrate_camera(ok.obj, ok.img, ok.size, K, np.zeros(14), flags=cv_hip.CALIB_USE_INTRINSIC_GUESS)
    assert e.value.code == camcallib.ERR_CAMERA
    # ... and the whole problem is accepted once it is complete
    gpu_solver(ok, cs.FREE5, 5).close()
    cc.calibrate_camera(ok.obj, ok.img, ok.size, max_iters=2)


def test_end_to_end_tool(tmp_path):
    """board recording -> tools/calibrate_camera.py -> CameraParams.npz -> PoseDetector on a clip of the body: every frame passes the
    2 px gate with the calibrated file, not every frame with the nominal one (focal length = image width, no distortion)"""
    import json
    import logging
    from accurate_aprilgroup_tracking_amd import formats, group_calib
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    board, frames = cs.e2e_board_recording()
    formats.save_detections(tmp_path / "board.npz", frames)
    with open(tmp_path / "board.json", "w") as f:
        json.dump(board, f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "calibrate_camera.py"), str(tmp_path / "board.npz"), str(tmp_path / "board.json"),
                        "--size", str(cs.E2E_SIZE[0]), str(cs.E2E_SIZE[1]), "-o", str(tmp_path / "CameraParams.npz")], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "final RMS" in r.stdout and "RMS view 14" in r.stdout
    mtx, dist, rvecs, tvecs = formats.load_camera_params(tmp_path / "CameraParams.npz")
    assert dist.shape == (1, 5) and rvecs.shape == tvecs.shape == (cs.E2E_BOARD_VIEWS, 3, 1)
    print("calibrated - true camera: %s" % np.array2string(np.concatenate([[mtx[0, 0], mtx[1, 1], mtx[0, 2], mtx[1, 2]], dist.ravel()]) - cs.E2E_CAM[:9], precision=3))
    formats.save_camera_params(tmp_path / "nominal.npz", *cs.e2e_nominal_camera())
    sc = cs.e2e_body_clip()
    formats.save_detections(tmp_path / "rec.npz", sc.frames)
    formats.save_april_group(tmp_path / "april_group.json", group_calib.poses_to_group(sc.tag_poses, sc.tag_ids, sc.sizes))
    log = logging.getLogger("camcal"); log.setLevel(logging.CRITICAL)
    accepted = {}
    for name in ("CameraParams.npz", "nominal.npz"):
        det = PoseDetector.from_files(log, tmp_path / name, True, detector=tmp_path / "rec.npz", april_group=tmp_path / "april_group.json")
        ok = []
        for _ in sc.frames:
            il, ol, _ = det._obtain_detections(None)
            det._estimate_pose(il, ol)
            ok.append(det.last_error is not None and det.last_error < det.ERROR_GATE_PX)
        accepted[name] = ok
    print("accepted frames: calibrated %d / %d, nominal %d / %d" % (sum(accepted["CameraParams.npz"]), len(sc.frames), sum(accepted["nominal.npz"]), len(sc.frames)))
    assert all(accepted["CameraParams.npz"])
    assert not all(accepted["nominal.npz"])
