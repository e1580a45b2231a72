"""Forward-backward check, the part that needs no GPU: the two entry points exist at every layer and refuse bad arguments without a
device, and the scenes of tests/fb_scenes.py are what the GPU tests take them for -- by the CPU oracle alone."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import fb_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("agt_lk_track_fb", "agt_tracker_fb_check")


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
    assert len(L.agt_lk_track_fb.argtypes) == 16 and len(L.agt_tracker_fb_check.argtypes) == 2
    ARG = -1
    # no context: refused before anything touches a device
    assert L.agt_tracker_fb_check(None, 1.0) == ARG
    assert L.agt_lk_track_fb(None, 0, 1, None, None, None, None, None, 48, 1, 3, 30, 0.01, 0, 1e-4, 1.0) == ARG
    # the threshold is judged before the context is used: a context that is never dereferenced stands in for one
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    for bad in (math.nan, math.inf, -math.inf, -1.0):
        assert L.agt_tracker_fb_check(h, bad) == ARG, bad
    for bad in (math.nan, math.inf, -math.inf, -1.0, 0.0):
        assert L.agt_lk_track_fb(h, 0, 1, None, None, None, None, None, 48, 1, 3, 30, 0.01, 0, 1e-4, bad) == ARG, bad
    # Python surface
    from accurate_aprilgroup_tracking_amd import cv_hip, tracker, pose_detector
    import inspect
    assert callable(cv_hip.Context.lk_track_fb) and callable(tracker.StreamTracker.fb_check)
    sig = inspect.signature(cv_hip.trackForwardBackward)
    assert list(sig.parameters)[:9] == ["prevImg", "nextImg", "prevPts", "winSize", "maxLevel", "criteria", "flags", "minEigThreshold",
                                        "fbThreshold"] and sig.parameters["fbThreshold"].default == 1.0
    assert inspect.signature(tracker.StreamTracker.__init__).parameters["fb_check"].default == 0.0
    assert inspect.signature(pose_detector.PoseDetector.__init__).parameters["lk_fb_px"].default is None


def _chains(oracle, sc):
    """plain LK chain and forward-backward chain over the scene -> per frame (error of the plain chain's corners against the
    exact projections, plain alive, checked alive, round-trip distances)"""
    n = sc.obj.shape[0]
    pts = sc.corners(0).copy(); alive = np.ones(n, bool)
    pts_fb = pts.copy(); alive_fb = alive.copy()
    out = []
    for k in range(1, len(sc)):
        a, b = sc.frame(k - 1), sc.frame(k)
        nx, st, _ = oracle.calcOpticalFlowPyrLK(a, b, pts, winSize=(S.WIN, S.WIN), maxLevel=S.MAX_LEVEL)
        nx = nx.reshape(-1, 2); nx[~alive] = pts[~alive]
        alive = alive & st.ravel().astype(bool)
        nf, st_fb, _, dist, _ = S.oracle_fb(oracle, a, b, pts_fb, alive=alive_fb)
        alive_fb = alive_fb & st_fb.astype(bool)
        out.append((np.abs(nx - sc.corners(k)).max(axis=1), alive.copy(), alive_fb.copy(), dist))
        pts, pts_fb = nx.astype(np.float32), nf.astype(np.float32)
    return out


def test_occluder_scene_is_not_vacuous(oracle):
    """720p scene: plain LK keeps status 1 on the four occluded corners with > 2 px of error; the composition of two oracle LK calls
    drops exactly those four from frame OCC_FROM on and no other corner in any frame."""
    sc = S.OccludedSequence(*S.SCENE_720P)
    tag0 = np.zeros(sc.obj.shape[0], bool); tag0[4 * S.OCC_TAG:4 * S.OCC_TAG + 4] = True
    for k, (err, alive, alive_fb, dist) in enumerate(_chains(oracle, sc), start=1):
        assert alive.all(), "frame %d: plain LK itself dropped a corner" % k
        if k < S.OCC_FROM:
            assert alive_fb.all() and err.max() < 1.0
            continue
        assert (err[tag0] > 2.0).all(), "frame %d: occluded corners off by only %s px" % (k, err[tag0])
        assert np.array_equal(~alive_fb, tag0), "frame %d: the check dropped corners %s" % (k, np.nonzero(~alive_fb)[0])
        assert dist[~tag0].max() < 0.1, "frame %d: a clean corner's round trip is %g px" % (k, dist[~tag0].max())
        if k == S.OCC_FROM:
            assert (dist[tag0] >= S.FB_PX).all()


# a clean pair is one LK itself gets right (every corner within 1 px of its exact projection).  The fast pair is seed 0: with seed 1
# at 2.4 x speed the two-frame jump is 19 px and plain LK already loses nine corners to neighbouring tags -- not a clean pair.
CLEAN_PAIRS = [(640, 480, 0, 1.0, 1), (1280, 720, 1, 1.0, 1), (1280, 720, 0, 2.4, 2)]


@pytest.mark.parametrize("width,height,seed,speed,jump", CLEAN_PAIRS)
def test_clean_pairs_lose_no_corner(oracle, width, height, seed, speed, jump):
    sc = S.OccludedSequence(width, height, seed, n_frames=jump + 1, occluded=False, speed=speed)
    nx, st, _, dist, st_f = S.oracle_fb(oracle, sc.frame(0), sc.frame(jump), sc.corners(0))
    assert st_f.all() and np.abs(nx - sc.corners(jump)).max() < 1.0, "not a clean pair"
    assert st.all(), "the check dropped corners %s of a clean pair (round trips %s)" % (np.nonzero(st == 0)[0], dist[st == 0])
    assert dist.max() < 0.5


def test_fb_rule_nan_and_lost():
    p = np.array([[1, 1], [2, 2], [3, 3], [4, 4]], np.float32)
    back = np.array([[1.5, 1], [np.nan, 2], [3, 3], [4, 5]], np.float32)
    st, d = S.fb_rule(p, back, [1, 1, 0, 1], [1, 1, 1, 1], 1.0)
    assert st.tolist() == [1, 0, 0, 0] and d[0] == 0.5 and np.isnan(d[1]) and d[2] == -1.0 and d[3] == 1.0
