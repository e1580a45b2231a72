"""CPU: the visibility rule of the reproject refresh (agt_tracker_visibility / agt_tag_visibility, include/agt_hip.h) -- its entry points
exist and refuse bad arguments without a device, and its numpy statement (tests/visibility_scenes.py tag_visibility, the expected
value of every GPU test in test_gpu_tag_visibility.py) agrees with the one place the project already knows the rule: the renderer
paints exactly the tags the rule sees at 90 degrees."""
import ctypes
import os

import numpy as np
import pytest

import visibility_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODIES = (12, 24)
STEPS = (S.STEP_DEG, -S.STEP_DEG)


def test_symbols_and_argument_errors_without_a_device():
    import __graft_entry__ as g
    g.build()
    from accurate_aprilgroup_tracking_amd import hiplib as H
    lib = ctypes.CDLL(H.LIB_PATH)
    for s in ("agt_tracker_visibility", "agt_tag_visibility"):
        assert hasattr(lib, s) and s in H.SYMBOLS
    assert H.ST_NVISIBLE == 13 and H.STATE_STRIDE == 16
    L = H.lib()
    assert L.agt_tracker_visibility(None, 4, 70.0, 1) == -1
    assert L.agt_tag_visibility(None, None, 0, H.F32, 48, 1, None, 4, 70.0, 1, None, None) == -1
    header = open(os.path.join(ROOT, "include", "agt_hip.h")).read()
    assert "#define AGT_ST_NVISIBLE 13" in header and "#define AGT_VERSION 505" in header


def test_python_entry_points_refuse_bad_arguments_before_they_need_a_device():
    from accurate_aprilgroup_tracking_amd import cv_hip
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    obj = S.ClosedBodyClip.get(12).obj
    r, t = np.zeros(3), np.array([0.0, 0.0, 0.3])
    for kw in (dict(maxViewDeg=0.0), dict(maxViewDeg=90.5), dict(maxViewDeg=float("nan")), dict(facing=0), dict(facing=2),
               dict(cornersPerTag=3), dict(cornersPerTag=5)):
        with pytest.raises(cv_hip.error):
            cv_hip.tagVisibility(obj, r, t, **kw)
    with pytest.raises(cv_hip.error):
        cv_hip.tagVisibility(obj[:46], r, t)
    with pytest.raises(cv_hip.error):
        cv_hip.tagVisibility(obj, np.zeros(4), t)
    # the rule acts in the reproject refresh only: a tracker without reproject must not accept it silently
    with pytest.raises(ValueError, match="reproject"):
        StreamTracker(S.WIDTH, S.HEIGHT, obj, np.eye(3), None, view_deg=70.0)
    with pytest.raises(ValueError, match="reproject"):
        StreamTracker(S.WIDTH, S.HEIGHT, obj, np.eye(3), None, reproject=False, view_deg=70.0, facing=-1)


def _painted(clip, k):
    """the tags synthetic.render_frame paints at pose k, asked of the renderer itself: tag by tag, the coverage it reports"""
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    out = []
    for ti, key in enumerate(clip.group["tags"]):
        cov = np.zeros((S.HEIGHT, S.WIDTH), np.float32)
        syn.render_frame({"tags": {key: clip.group["tags"][key]}}, clip.bits[ti:ti + 1], clip.rvecs[k], clip.tvecs[k], clip.K, None,
                         S.WIDTH, S.HEIGHT, clip.bg, 1, cover_out=cov)
        out.append(bool(cov.sum() > 0))
    return np.array(out)


@pytest.mark.parametrize("n_tags", BODIES)
def test_rule_at_90_degrees_is_what_the_renderer_paints(oracle, n_tags):
    judged = hidden = shown = 0
    for step in STEPS:
        clip = S.ClosedBodyClip.get(n_tags, step)
        for k in range(0 if step > 0 else 1, len(clip), 3):          # (frame 0 is the same pose in both clips)
            vis, cs, z = S.tag_visibility(clip.obj, clip.rvecs[k], clip.tvecs[k], 4, 90.0, 1)
            sure = np.abs(cs) > 1e-6
            painted = _painted(clip, k)
            assert np.array_equal(vis[sure], painted[sure]), "%d tags, step %g, frame %d: rule %s, renderer %s" % (n_tags, step, k, vis, painted)
            assert (z > 0).all()
            judged += int(sure.sum()); shown += int(vis.sum()); hidden += int((~vis).sum())
    # a closed body: a good part of the tags faces away at every pose, and every tag was judged
    assert judged == shown + hidden and shown >= judged // 4 and hidden >= judged // 4


@pytest.mark.parametrize("n_tags", BODIES)
def test_facing_minus_one_is_the_complement_in_front_of_the_camera(oracle, n_tags):
    clip = S.ClosedBodyClip.get(n_tags)
    obj32 = clip.obj.astype(np.float32)
    poses = [(clip.rvecs[k], clip.tvecs[k]) for k in (0, 5, 15)]
    poses.append((clip.rvecs[3], np.array([0.01, -0.01, 0.01])))       # the camera inside the body: some tag centres behind it
    behind = 0
    for r, t in poses:
        for deg in (90.0, 70.0):
            vp, cp, zp = S.tag_visibility(obj32, r, t, 4, deg, 1)
            vm, cm, zm = S.tag_visibility(obj32, r, t, 4, deg, -1)
            assert np.array_equal(cp, -cm) and np.array_equal(zp, zm)
            assert not (vp & vm).any() and not vp[zp <= 0].any() and not vm[zp <= 0].any()
            if deg == 90.0:
                sure = (np.abs(cp) > 1e-6) & (zp > 0)
                assert np.array_equal(vm[sure], ~vp[sure])
            else:
                # below 90 degrees a band of tags near the limb is hidden under either sign
                th = S.cos_threshold(deg)
                assert np.array_equal(vp, (zp > 0) & (cp > th)) and np.array_equal(vm, (zp > 0) & (-cp > th))
        behind += int((zp <= 0).sum())
    assert behind > 0


def test_threshold_is_exactly_zero_at_90_degrees():
    assert S.cos_threshold(90.0) == 0.0 and abs(S.cos_threshold(60.0) - 0.5) < 1e-15 and 0.0 < S.cos_threshold(89.999) < 2e-5
