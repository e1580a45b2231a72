"""CPU: the camera-calibration library (include/agt_camcal.h -> libagt_camcal.so) builds, exports exactly its header, keeps its
kernels out of scratch and judges its arguments without a device; the numpy / scipy statement of the problem
(tests/camera_calib_numpy.py) that the GPU tests compare with is sound (its Jacobian is the derivative, Schur step = dense step, scipy
recovers the truth); the host parts of camera_calib.py (focal closed form, flag mapping, recording -> point lists) and the premise of
the end-to-end GPU test."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import camcal_scenes as cs         # noqa: E402
import camera_calib_numpy as cn    # noqa: E402
import pnp_numpy                   # noqa: E402

KERNELS = ["camcal_accumulate_kernel", "camcal_backsub_kernel", "camcal_cost_kernel", "camcal_eliminate_kernel", "camcal_reduce_kernel"]
LAMBDAS = (0.0, 1e-3, 10.0)


def numpy_start(sc):
    """cv2's start without a guess, on the host: centre, closed-form focal lengths, no distortion; poses by the planar solvePnP statement"""
    from accurate_aprilgroup_tracking_amd import camera_calib as cc
    c0 = np.zeros(16)
    c0[2], c0[3] = (sc.size[0] - 1) / 2.0, (sc.size[1] - 1) / 2.0
    c0[0], c0[1] = cc.initial_focal_lengths(sc.obj, sc.img, (c0[2], c0[3]))
    return c0, numpy_poses(sc, c0)


def numpy_poses(sc, c):
    K, _ = cn.split(c)
    return np.array([np.concatenate(pnp_numpy.solve_pnp_noguess_planar(X, m, K, None)[:2]) for X, m in zip(sc.obj, sc.img)])


def test_camcal_library_builds_exports_and_resources():
    import side_library
    from accurate_aprilgroup_tracking_amd import camcallib
    rows = side_library.built(camcallib, "camcal")
    assert [re.search(r"(camcal_\w+)\(", r["name"]).group(1) for r in rows] == KERNELS
    bad = [(r["name"], r["scratch"], r["vgpr"], r["vspill"]) for r in rows if r["scratch"] != 0 or r["vgpr"] > 512 or r["vspill"] != 0]
    assert not bad, bad
    assert camcallib.lib().agt_camcal_version() == camcallib.VERSION == 100


def test_argument_errors_need_no_device():
    from accurate_aprilgroup_tracking_amd import camcallib
    L = camcallib.lib()
    h = ctypes.c_void_p()
    assert L.agt_camcal_create(None, None, ctypes.byref(h)) == camcallib.ERR_ARG
    assert L.agt_camcal_destroy(None) == 0

    def create(counts, free, ndist, **null):
        start, X, m = camcallib.pack_views([np.zeros((n, 3)) for n in counts], [np.zeros((n, 2)) for n in counts])
        p = camcallib.Problem(len(counts), ndist, free, 0, None if "start" in null else start.ctypes.data, None if "obj" in null else X.ctypes.data,
                              None if "img" in null else m.ctypes.data)
        rc = L.agt_camcal_create(ctypes.byref(p), None, ctypes.byref(h))
        assert not h.value
        return rc
    for k in ("start", "obj", "img"):
        assert create([6, 6, 6], 0x1FF, 5, **{k: True}) == camcallib.ERR_ARG
    assert create([6, 3, 6], 0x3, 5) == camcallib.ERR_ARG                    # a 3-point view
    assert create([6, 4097, 6], 0x3, 5) == camcallib.ERR_ARG
    assert create([6, 6, 6], 0x1FFFF, 12) == camcallib.ERR_ARG               # a 17th entry
    # 3 views of 4 points: 24 residuals.  18 pose unknowns + 6 camera entries pass, + 7 do not
    assert create([4, 4, 4], 0x7F, 5) == camcallib.ERR_TOO_FEW
    assert create([4, 4, 4], 0x1FF, 14) == camcallib.ERR_CAMERA              # (the model is judged before the count)
    assert create([6, 6, 6], 0x1FF, 14) == camcallib.ERR_CAMERA              # the tilted model
    assert create([6, 6, 6], 0x1FF, 6) == camcallib.ERR_CAMERA
    assert create([6, 6, 6], 0x3FF, 5) == camcallib.ERR_CAMERA               # k4 free in a 5-coefficient model


def test_missing_library_raises(monkeypatch):
    from accurate_aprilgroup_tracking_amd import camcallib
    monkeypatch.setattr(camcallib, "_lib", None)
    monkeypatch.setattr(camcallib, "LIB_PATH", "/nonexistent/libagt_camcal.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        camcallib.lib()


def test_numpy_jacobian_is_the_derivative():
    """all 22 columns, every one of the 16 camera entries non-zero"""
    sc = cs.parity_scene(cs.CAM12)
    assert np.all(sc.cam != 0.0)
    prob = sc.problem(range(16))
    c, p = cs.perturbed_start(sc, range(16))
    _, J = cn.jacobian(prob, c, p)
    for j in range(16):
        h = 1e-6 * max(1.0, abs(c[j]))
        a, b = c.copy(), c.copy()
        a[j] += h; b[j] -= h
        num = (cn.residuals(prob, a, p) - cn.residuals(prob, b, p)).ravel() / (2 * h)
        assert np.abs(num - J[:, j]).max() < 1e-6 * max(1.0, np.abs(J[:, j]).max()), j
    for v in range(len(sc.obj)):
        for j in range(6):
            h = 1e-6
            a, b = p.copy(), p.copy()
            a[v, j] += h; b[v, j] -= h
            num = (cn.residuals(prob, c, a) - cn.residuals(prob, c, b)).ravel() / (2 * h)
            col = J[:, 16 + 6 * v + j]
            assert np.abs(num - col).max() < 1e-6 * max(1.0, np.abs(col).max()), (v, j)


STEP_CASES = {"coeff5": (lambda: cs.parity_scene(cs.CAM5), cs.FREE5, LAMBDAS), "prism": (lambda: cs.parity_scene(cs.CAM12), cs.FREE_PRISM, LAMBDAS),
              "rational": (lambda: cs.parity_scene(cs.CAM8), cs.FREE8, LAMBDAS[1:]), "smallest": (cs.smallest_scene, [0, 1], LAMBDAS),
              "tile": (cs.tile_scene, cs.FREE5, LAMBDAS)}


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_numpy_schur_step_equals_dense_step(name):
    """the difference measured here is the floor of the GPU step tolerance (tests/test_gpu_camera_calib.py)"""
    make, free, lams = STEP_CASES[name]
    sc = make()
    prob = sc.problem(free)
    c, p = cs.perturbed_start(sc, free)
    print("%s: scaled condition of J %.3g" % (name, cn.scaled_condition(prob, c, p)))
    for lam in lams:
        d = cn.step_difference(cn.schur_step(prob, c, p, lam), cn.dense_step(prob, c, p, lam))
        print("%s lambda %g: |schur - dense| / |dense| = %.3g" % (name, lam, d))
        assert d < 1e-8


def test_scene_builders():
    assert [len(o) for o in cs.tile_scene().obj] == list(cs.TILE_COUNTS)
    sc = cs.smallest_scene()
    assert len(sc.obj) == 3 and all(len(o) == 4 for o in sc.obj)
    for sc in (cs.parity_scene(cs.CAM12), cs.recovery_scene()):
        # tilted 17-35 degrees: the angle between the target's normal and the optical axis
        tilt = np.rad2deg([np.arccos(pnp_numpy.rodrigues(p[:3])[0][2, 2]) for p in sc.poses])
        assert tilt.min() >= 17.0 - 1e-9 and tilt.max() <= 35.0 + 1e-9
        assert np.abs(cn.residuals(sc.problem(cs.FREE5), sc.cam, sc.poses)).max() == 0.0
    assert np.any(cs.nonplanar_scene().obj[0][:, 2] != 0.0)
    assert all(np.arccos(pnp_numpy.rodrigues(p[:3])[0][2, 2]) < 1e-12 for p in cs.fronto_scene().poses)


def test_focal_closed_form_and_numpy_recovery():
    """the closed form lands within 5 % on the noise-free recovery scene, and scipy reaches the truth from it and from a 5 % start"""
    sc = cs.recovery_scene()
    prob = sc.problem(cs.FREE5)
    c0, p0 = numpy_start(sc)
    print("closed form: fx %.3f fy %.3f (truth %.1f %.1f)" % (c0[0], c0[1], sc.cam[0], sc.cam[1]))
    assert abs(c0[0] / sc.cam[0] - 1) < 0.05 and abs(c0[1] / sc.cam[1] - 1) < 0.05
    c5 = c0.copy()
    c5[0], c5[1] = 1.05 * sc.cam[0], 0.95 * sc.cam[1]
    for name, (ca, pa) in (("closed form", (c0, p0)), ("5 % start", (c5, numpy_poses(sc, c5)))):
        c, p, cost, rms = cn.solve(prob, ca, pa)
        print("%s: scipy vs truth: camera %.3g poses %.3g rms %.3g" % (name, np.abs(c - sc.cam).max(), np.abs(p - sc.poses).max(), rms))
        assert np.abs(c - sc.cam).max() < 1e-9 and np.abs(p - sc.poses).max() < 1e-10 and rms < 1e-10
        assert np.array_equal(c[9:], sc.cam[9:])         # the fixed entries stay


def test_numpy_recovers_the_smallest_and_the_prism_scene():
    for make, free in ((cs.smallest_scene, [0, 1]), (lambda: cs.parity_scene(cs.CAM12), cs.FREE_PRISM)):
        sc = make()
        c0, p0 = cs.perturbed_start(sc, free)
        c, p, cost, rms = cn.solve(sc.problem(free), c0, p0)
        print("scipy vs truth: camera %.3g poses %.3g rms %.3g" % (np.abs(c - sc.cam).max(), np.abs(p - sc.poses).max(), rms))
        assert np.abs(c - sc.cam).max() < 1e-7 and rms < 1e-9


def test_degenerate_starts_are_refused():
    from accurate_aprilgroup_tracking_amd import camcallib, camera_calib as cc
    sc = cs.fronto_scene()
    with pytest.raises(camcallib.CamCalError) as e:
        cc.initial_focal_lengths(sc.obj, sc.img, (319.5, 239.5))
    assert e.value.code == camcallib.ERR_DEGENERATE
    # two views or a lifted target without a guess: refused before anything touches a device
    two = cs.recovery_scene().subset([0, 1])
    with pytest.raises(camcallib.CamCalError) as e:
        cc.calibrate_camera(two.obj, two.img, two.size)
    assert e.value.code == camcallib.ERR_TOO_FEW
    sc = cs.nonplanar_scene()
    with pytest.raises(camcallib.CamCalError) as e:
        cc.calibrate_camera(sc.obj, sc.img, sc.size)
    assert e.value.code == camcallib.ERR_ARG


def test_flags_to_mask():
    from accurate_aprilgroup_tracking_amd import camera_calib as cc, cv_hip
    bits = lambda *names: sum(1 << cc.camcallib.CAMERA_NAMES.index(n) for n in names)
    base = bits("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")
    assert cc.flags_to_mask(0) == (base, 5)
    assert cc.flags_to_mask(cv_hip.CALIB_USE_INTRINSIC_GUESS) == (base, 5)
    assert cc.flags_to_mask(cv_hip.CALIB_FIX_PRINCIPAL_POINT) == (base & ~bits("cx", "cy"), 5)
    assert cc.flags_to_mask(cv_hip.CALIB_FIX_FOCAL_LENGTH) == (base & ~bits("fx", "fy"), 5)
    assert cc.flags_to_mask(cv_hip.CALIB_ZERO_TANGENT_DIST) == (base & ~bits("p1", "p2"), 5)
    for i, f in enumerate((cv_hip.CALIB_FIX_K1, cv_hip.CALIB_FIX_K2, cv_hip.CALIB_FIX_K3, cv_hip.CALIB_FIX_K4, cv_hip.CALIB_FIX_K5, cv_hip.CALIB_FIX_K6)):
        full = base | bits("k4", "k5", "k6")
        assert cc.flags_to_mask(cv_hip.CALIB_RATIONAL_MODEL | f) == (full & ~bits("k%d" % (i + 1)), 8)
    assert cc.flags_to_mask(cv_hip.CALIB_FIX_K4) == (base, 5)
    assert cc.flags_to_mask(cv_hip.CALIB_RATIONAL_MODEL) == (base | bits("k4", "k5", "k6"), 8)
    assert cc.flags_to_mask(cv_hip.CALIB_THIN_PRISM_MODEL) == (base | bits("s1", "s2", "s3", "s4"), 12) == (cn.mask_of(dict(free=cs.FREE_PRISM)), 12)
    assert cc.flags_to_mask(cv_hip.CALIB_THIN_PRISM_MODEL | cv_hip.CALIB_RATIONAL_MODEL) == (0xFFFF, 12)
    assert cc.flags_to_mask(cv_hip.CALIB_THIN_PRISM_MODEL | cv_hip.CALIB_FIX_S1_S2_S3_S4) == (base, 12)
    for name in ("CALIB_TILTED_MODEL", "CALIB_FIX_ASPECT_RATIO", "CALIB_USE_QR", "CALIB_USE_LU"):
        with pytest.raises(cv_hip.error, match=name):
            cc.flags_to_mask(getattr(cv_hip, name))
        with pytest.raises(cv_hip.error, match=name):
            cv_hip.calibrateCamera([], [], (640, 480), None, None, flags=getattr(cv_hip, name))


def test_target_points_from_detections_filters():
    from accurate_aprilgroup_tracking_amd import camera_calib as cc, formats
    board = cs.e2e_board()
    c = np.arange(8.0).reshape(4, 2)
    frames = [[formats.make_detection(3, c), formats.make_detection(5, c + 1, decision_margin=10.0), formats.make_detection(99, c)],
              [], [formats.make_detection(5, c + 2), formats.make_detection(5, c + 3), formats.make_detection(0, c + 4)]]
    obj, img, used = cc.target_points_from_detections(frames, board)
    assert used == [0, 2] and [len(o) for o in obj] == [4, 8]
    assert np.array_equal(img[0], c) and np.array_equal(img[1], np.concatenate([c + 3, c + 4]))
    r = 0.015
    corners = np.array([[-r, -r, 0.0], [-r, r, 0.0], [r, r, 0.0], [r, -r, 0.0]])
    centre = lambda t: np.array(board["tags"][str(t)]["extrinsics"][:3])
    assert np.allclose(obj[0], corners + centre(3), atol=1e-9) and np.allclose(obj[1], np.concatenate([corners + centre(5), corners + centre(0)]), atol=1e-9)
    assert all(np.all(o[:, 2] == 0.0) for o in obj)
    # a board in a plane z = const is moved to z = 0; a board that is not flat is refused
    lifted = {"tags": {k: dict(v, extrinsics=[*v["extrinsics"][:2], 0.25, 0, 0, 0]) for k, v in board["tags"].items()}}
    assert np.array_equal(cc.target_points_from_detections(frames, lifted)[0][0], obj[0])
    bent = {"tags": dict(board["tags"], **{"0": {"size": 0.03, "extrinsics": [0, 0, 0.01, 0.3, 0, 0]}})}
    with pytest.raises(ValueError, match="plane"):
        cc.target_points_from_detections(frames, bent)


def test_camera_params_round_trip_with_view_poses(tmp_path):
    from accurate_aprilgroup_tracking_amd import camera_calib as cc, formats
    sc = cs.recovery_scene()
    mtx, dist = cc.camera_from_vector(sc.cam + 1e-9, 5)
    formats.save_camera_params(tmp_path / "CameraParams.npz", mtx, dist, sc.poses[:, :3].reshape(-1, 3, 1), sc.poses[:, 3:].reshape(-1, 3, 1))
    m2, d2, rv, tv = formats.load_camera_params(tmp_path / "CameraParams.npz")
    assert np.array_equal(m2, mtx) and d2.shape == (1, 5) and np.array_equal(d2, dist)
    assert rv.shape == tv.shape == (len(sc.poses), 3, 1)
    assert np.array_equal(rv.reshape(-1, 3), sc.poses[:, :3]) and np.array_equal(tv.reshape(-1, 3), sc.poses[:, 3:])
    assert np.array_equal(cc.camera_vector(m2, d2)[:9], (sc.cam + 1e-9)[:9])


def test_nominal_camera_fails_the_gate():
    """the premise of the end-to-end GPU test, confirmed with the numpy solvePnP: on the clip of the body a nominal camera (focal
    length = the image width, no distortion) fails the 2 px gate (mean corner error of the solved pose) on at least one frame, the true
    camera on none"""
    from accurate_aprilgroup_tracking_amd import group_calib
    sc = cs.e2e_body_clip()
    obj = group_calib.object_points(sc.tag_poses, sc.sizes).reshape(-1, 4, 3)
    Kt, dt = cn.split(cs.E2E_CAM)
    worst = {}
    for name, (K, dist) in (("truth", (Kt, dt[:5])), ("nominal", cs.e2e_nominal_camera())):
        errs = []
        for f, dets in enumerate(sc.frames):
            o = obj[[sc.tag_ids.index(d.tag_id) for d in dets]].reshape(-1, 3); img = np.concatenate([d.corners for d in dets])
            r, t, _ = pnp_numpy.solve_pnp_guess(o, img, K, dist, sc.frame_poses[f, :3], sc.frame_poses[f, 3:])
            errs.append(np.linalg.norm(pnp_numpy.project(o, r, t, K, dist) - img, axis=1).mean())
        worst[name] = max(errs)
    print("worst mean reprojection error: truth %.3g px, nominal %.3g px" % (worst["truth"], worst["nominal"]))
    assert worst["truth"] < 1e-3 and worst["nominal"] > 2.0
