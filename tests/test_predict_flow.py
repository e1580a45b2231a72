"""Motion-predicted initial flow, the part that needs no GPU: the fast scenes of tests/predict_scenes.py are what the GPU tests take them
for -- by the oracle-backed host mirror alone --, the host rule (pose_detector.predict_flow) does what include/agt_hip.h says, and the two
entry points exist at every layer and refuse bad arguments without a device."""
import ctypes as C
import inspect
import logging
import math
import os
import re

import numpy as np
import pytest

import predict_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = logging.getLogger("predict")
NEW = ("agt_predict_flow", "agt_tracker_predict")


# ---------------------------------------------------------------------------------------------------------------- the scenes
def _run(tmp_path, sc, tag, **options):
    """the oracle-backed mirror over the scene, first frame detector-fed -> per frame (last_error or None, tvec or None, tags kept)"""
    from oracle import cv2_shim
    det = S.detector_class(tmp_path, sc, tag)(LOG, sc.K, sc.dist, True, cv=cv2_shim.make_cv2(), detector=S.FirstFrameDetector(sc), **options)
    out = []
    for k in range(len(sc)):
        det._detect_and_get_pose(sc.frame(k))
        tv = None if det.last_pose[1] is None else np.array(det.last_pose[1], np.float64).ravel()       # (a copy: solvePnP writes into guess arrays)
        out.append((det.last_error, tv, len(det._prev_ids or [])))
    return out


@pytest.mark.parametrize("spec", [S.FAST_480, S.FAST_720], ids=["fast_480", "fast_720"])
def test_fast_scenes_are_not_vacuous(tmp_path, oracle, spec):
    """Plain LK loses the body from frame 3 on (with or without the forward-backward check); with the predicted flow every frame is
    accepted, on FAST_720 within 0.5 mm of the true translation, and the check drops nothing after frames 1-2."""
    sc = S.scene(spec)
    plain = _run(tmp_path, sc, "plain")
    pred = _run(tmp_path, sc, "pred", lk_predict_px=S.CAP_PX)
    fb = _run(tmp_path, sc, "fb", lk_fb_px=1.0)
    both = _run(tmp_path, sc, "both", lk_fb_px=1.0, lk_predict_px=S.CAP_PX)
    for k in range(len(sc)):
        print("frame %d: plain %s  predicted %s  fb %s (%d tags)  fb+predicted %s (%d tags)  tvec off %s mm" % (
            k, plain[k][0], pred[k][0], fb[k][0], fb[k][2], both[k][0], both[k][2],
            None if pred[k][1] is None else 1e3 * np.abs(pred[k][1] - sc.tvecs[k]).max()))
    for k in range(len(sc)):
        assert pred[k][0] is not None and pred[k][0] < 2, "frame %d with the predicted flow: %s" % (k, pred[k][0])
        assert both[k][0] is not None and both[k][0] < 2, "frame %d with the check and the predicted flow: %s" % (k, both[k][0])
        if spec is S.FAST_720:
            assert np.abs(pred[k][1] - sc.tvecs[k]).max() < 0.5e-3, "frame %d: tvec %g mm off" % (k, 1e3 * np.abs(pred[k][1] - sc.tvecs[k]).max())
        if k >= 3:
            assert plain[k][0] is None or plain[k][0] >= 2, "frame %d: the plain chain is accepted (%g px)" % (k, plain[k][0])
            assert fb[k][0] is None, "frame %d: the checked plain chain still has a pose" % k
            assert both[k][2] >= both[2][2], "frame %d: the check dropped tags after frame 2 (%d -> %d)" % (k, both[2][2], both[k][2])


# ---------------------------------------------------------------------------------------------------------------- the host rule
def _screw(k):
    """pose k of a constant screw motion in the camera frame: T_k = M^k T_0"""
    from scipy.spatial.transform import Rotation
    Rm = Rotation.from_rotvec([0.02, -0.03, 0.05]).as_matrix(); tm = np.array([0.004, -0.002, 0.006])
    R = Rotation.from_rotvec([0.2, -0.1, 0.3]).as_matrix(); t = np.array([0.01, -0.02, 0.30])
    for _ in range(k):
        R, t = Rm @ R, Rm @ t + tm
    return Rotation.from_matrix(R).as_rotvec().reshape(3, 1), t.reshape(3, 1)


@pytest.fixture(scope="module")
def rule_case(oracle):
    from oracle import cv2_shim
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    group = syn.make_april_group(n_tags=12, seed=3)
    obj = syn.group_object_points(group).astype(np.float32)
    K = syn.camera_matrix(640, 480)
    older, newer = _screw(0), _screw(1)
    prev = np.asarray(oracle.projectPoints(obj.astype(np.float64), newer[0], newer[1], K, syn.MILD_DIST)[0], np.float64).reshape(-1, 2).astype(np.float32)
    return cv2_shim.make_cv2(), obj, K, syn.MILD_DIST, older, newer, prev


def test_rule_predicts_a_constant_screw_motion_exactly(oracle, rule_case):
    from accurate_aprilgroup_tracking_amd.pose_detector import predict_flow
    cv, obj, K, dist, older, newer, prev = rule_case
    seeds, flow, fmax, (rp, tp) = predict_flow(cv, obj, prev, older, newer, K, dist, None, 64.0)
    r3, t3 = _screw(2)
    assert np.abs(rp - r3).max() < 1e-12 and np.abs(tp - t3).max() < 1e-12
    o64 = obj.astype(np.float64)
    p1 = np.asarray(oracle.projectPoints(o64, newer[0], newer[1], K, dist)[0], np.float64).reshape(-1, 2)
    p3 = np.asarray(oracle.projectPoints(o64, rp, tp, K, dist)[0], np.float64).reshape(-1, 2)
    assert flow.dtype == np.float32 and np.array_equal(flow, (p3 - p1).astype(np.float32))
    assert seeds.dtype == np.float32 and np.array_equal(seeds, prev + flow)
    assert fmax == float(np.abs(flow).max()) and 1.0 < fmax < 64.0
    # the same numbers as the statement of the rule the GPU tests compare the device with
    s2, f2, m2, pose2 = S.flow_rule(oracle, obj, prev, np.concatenate([older[0].ravel(), older[1].ravel()]),
                                    np.concatenate([newer[0].ravel(), newer[1].ravel()]), K, dist)
    assert np.array_equal(s2, seeds) and np.array_equal(f2, flow) and m2 == fmax and np.array_equal(pose2, np.concatenate([rp.ravel(), tp.ravel()]))


def test_rule_distrust_and_mask(oracle, rule_case):
    from accurate_aprilgroup_tracking_amd.pose_detector import predict_flow
    cv, obj, K, dist, older, newer, prev = rule_case
    n = obj.shape[0]
    _, flow, fmax, _ = predict_flow(cv, obj, prev, older, newer, K, dist, None, 64.0)
    # a cap below the largest flow
    seeds, f, m, _ = predict_flow(cv, obj, prev, older, newer, K, dist, None, fmax * 0.999)
    assert m == -1.0 and seeds.tobytes() == prev.tobytes() and not f.any()
    # the cap itself is allowed
    assert predict_flow(cv, obj, prev, older, newer, K, dist, None, fmax)[2] == fmax
    # a corner behind the camera under the predicted pose: the body flies through the camera plane
    fly = (newer[0], newer[1] - np.array([[0.0], [0.0], [0.29]]))
    seeds, f, m, _ = predict_flow(cv, obj, prev, older, fly, K, dist, None, 1e9)
    assert m == -1.0 and seeds.tobytes() == prev.tobytes() and not f.any()
    # a NaN pose
    bad = (np.array([[np.nan], [0.0], [0.0]]), newer[1])
    seeds, f, m, pose = predict_flow(cv, obj, prev, older, bad, K, dist, None, 64.0)
    assert m == -1.0 and seeds.tobytes() == prev.tobytes() and not f.any() and np.isnan(pose[0]).all()
    # masked corners keep their position and do not count; an objecting corner that is masked does not object
    usable = np.ones(n, bool); usable[[0, 5, 17]] = False
    seeds, f, m, _ = predict_flow(cv, obj, prev, older, newer, K, dist, usable, 64.0)
    assert seeds[~usable].tobytes() == prev[~usable].tobytes() and not f[~usable].any()
    assert np.array_equal(seeds[usable], (prev + flow)[usable]) and m == float(np.abs(flow[usable]).max())
    worst = int(np.abs(flow).max(axis=1).argmax())
    usable = np.ones(n, bool); usable[worst] = False
    second = float(np.abs(flow[usable]).max())
    assert predict_flow(cv, obj, prev, older, newer, K, dist, usable, (second + fmax) / 2)[2] == second
    assert predict_flow(cv, obj, prev, older, newer, K, dist, np.zeros(n, bool), 64.0)[2] == 0.0
    for cap in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            predict_flow(cv, obj, prev, older, newer, K, dist, None, cap)


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_symbols_declared_exported_bound_and_argument_errors():
    from accurate_aprilgroup_tracking_amd import hiplib as H
    header = open(os.path.join(ROOT, "include", "agt_hip.h")).read()
    vmap = open(os.path.join(ROOT, "accurate_aprilgroup_tracking_amd", "csrc", "agt_hip.map")).read()
    L = H.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), "%s is not declared in include/agt_hip.h" % name
        assert re.search(r"^\s*%s;" % name, vmap, re.M), "%s is not in agt_hip.map" % name
        assert name in H.SYMBOLS and hasattr(L, name)
    assert L.agt_version() == 505
    assert re.search(r"#define\s+AGT_ST_FLOW\s+15\b", header) and H.ST_FLOW == 15
    assert len(L.agt_predict_flow.argtypes) == 18 and len(L.agt_tracker_predict.argtypes) == 2
    ARG, NPOINTS = -1, -4
    assert L.agt_tracker_predict(None, 64.0) == ARG
    # the arguments are judged before the context is used: a context that is never dereferenced stands in for one
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    p = C.cast(C.create_string_buffer(64), C.c_void_p)          # (a non-null pointer that is never followed)
    for bad in (math.nan, math.inf, -math.inf, -1.0):
        assert L.agt_tracker_predict(h, bad) == ARG, bad
    call = lambda ctx, obj, older, newer, prev, seed, n, cap: L.agt_predict_flow(ctx, obj, 0, H.F32, n, 1, older, newer, None, None, 0, prev, None, cap,
                                                                                seed, None, None, None)
    assert call(None, p, p, p, p, p, 48, 64.0) == ARG
    for k in range(5):
        args = [p] * 5
        args[k] = None
        assert call(h, *args, 48, 64.0) == ARG, "NULL pointer %d" % k
    for bad in (math.nan, math.inf, -math.inf, -1.0, 0.0):
        assert call(h, p, p, p, p, p, 48, bad) == ARG, bad
    assert call(h, p, p, p, p, p, 257, 64.0) == NPOINTS


def test_python_surface():
    from accurate_aprilgroup_tracking_amd import cv_hip, tracker, pose_detector
    assert callable(cv_hip.Context.predict_flow) and callable(tracker.StreamTracker.predict)
    sig = inspect.signature(cv_hip.predictFlow)
    assert list(sig.parameters) == ["objectPoints", "rvecOlder", "tvecOlder", "rvecNewer", "tvecNewer", "cameraMatrix", "distCoeffs", "prevPts",
                                    "mask", "maxFlow"]
    assert sig.parameters["mask"].default is None and sig.parameters["maxFlow"].default == 64.0
    assert inspect.signature(tracker.StreamTracker.__init__).parameters["predict_px"].default == 0.0
    assert inspect.signature(pose_detector.PoseDetector.__init__).parameters["lk_predict_px"].default is None
    assert inspect.signature(pose_detector.PoseDetector.from_files).parameters["lk_predict_px"].default is None
    assert list(inspect.signature(pose_detector.predict_flow).parameters) == ["cv", "obj", "prev_pts", "older", "newer", "mtx", "dist", "usable",
                                                                              "max_flow_px"]
    K = np.array([[600.0, 0, 320], [0, 600.0, 240], [0, 0, 1]])
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            pose_detector.PoseDetector(LOG, K, None, True, cv=object(), lk_predict_px=bad)
        # (the tracker judges its threshold before it creates a context: no device is needed to be refused)
        with pytest.raises(ValueError):
            tracker.StreamTracker(640, 480, np.zeros((48, 3)), K, predict_px=bad)
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(cv_hip.error):
            cv_hip.predictFlow(np.zeros((4, 3), np.float32), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3), K, None, np.zeros((4, 2), np.float32),
                               maxFlow=bad)
