"""Tag-consensus PnP, the part that needs no GPU: the entry points exist at every layer and refuse bad arguments without a device, the
host rule of PoseDetector(backend="cv") is the plain numpy statement of the rule (tests/consensus_scenes.py), and every scene of these
tests -- CPU and GPU -- meets the margin condition under the CPU oracle alone."""
import ctypes as C
import inspect
import json
import logging
import math
import os
import re

import numpy as np
import pytest

import consensus_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("agt_solve_pnp_consensus", "agt_tracker_consensus")
LOG = logging.getLogger("test"); LOG.setLevel(logging.CRITICAL)
ARG, NPOINTS = -1, -4


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
    assert re.search(r"#define\s+AGT_ST_NINLIER\s+14\b", header) and H.ST_NINLIER == 14 and H.STATE_STRIDE == 16
    assert len(L.agt_solve_pnp_consensus.argtypes) == 20 and len(L.agt_tracker_consensus.argtypes) == 4
    assert H.AgtError(ARG, "x").code == ARG
    # the arguments are judged before the context or any pointer is used: buffers that are never dereferenced stand in for them
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    K = (C.c_double * 9)(500, 0, 320, 0, 500, 240, 0, 0, 1)

    def call(n=48, cpt=4, px=2.0, mi=8, inl=h, ctx=h):
        return L.agt_solve_pnp_consensus(ctx, h, 0, h, H.F32, None, n, 1, K, None, 0, h, 0, cpt, px, mi, inl, None, None, None)
    assert call(ctx=None) == ARG
    for bad in (math.nan, math.inf, -math.inf, -1.0, 0.0):
        assert call(px=bad) == ARG, bad
    assert call(cpt=3) == ARG and call(n=46) == ARG and call(mi=3) == ARG and call(inl=None) == ARG
    assert call(n=260) == NPOINTS                             # n > 256 (and 65 tags)
    for bad in (math.nan, math.inf, -math.inf, -1.0):
        assert L.agt_tracker_consensus(h, 4, bad, 8) == ARG, bad
    assert L.agt_tracker_consensus(None, 4, 2.0, 8) == ARG
    assert L.agt_tracker_consensus(h, 3, 2.0, 8) == ARG and L.agt_tracker_consensus(h, 4, 2.0, 3) == ARG
    # Python surface
    from accurate_aprilgroup_tracking_amd import cv_hip, tracker, pose_detector
    assert callable(cv_hip.Context.solve_pnp_consensus) and callable(tracker.StreamTracker.consensus)
    sig = inspect.signature(cv_hip.solvePnPTagConsensus)
    assert list(sig.parameters) == ["objectPoints", "imagePoints", "cameraMatrix", "distCoeffs", "rvec", "tvec", "useExtrinsicGuess",
                                    "cornersPerTag", "reprojectionError", "minInliers"]
    assert (sig.parameters["cornersPerTag"].default, sig.parameters["reprojectionError"].default, sig.parameters["minInliers"].default) == (4, 2.0, 8)
    p = inspect.signature(tracker.StreamTracker.__init__).parameters
    assert p["consensus_px"].default == 0.0 and p["consensus_min"].default == 8
    assert inspect.signature(pose_detector.PoseDetector.__init__).parameters["pnp_consensus_px"].default is None
    assert inspect.signature(pose_detector.PoseDetector.from_files).parameters["pnp_consensus_px"].default is None


def test_python_argument_errors_are_value_errors(tmp_path):
    """judged before a device is needed"""
    from accurate_aprilgroup_tracking_amd import cv_hip
    sc = S.Scene(12, 0, 0)
    obj, img = sc.obj, sc.img()
    for kw in (dict(reprojectionError=0.0), dict(reprojectionError=-1.0), dict(reprojectionError=math.nan), dict(reprojectionError=math.inf),
               dict(cornersPerTag=3), dict(cornersPerTag=5), dict(minInliers=3), dict(useExtrinsicGuess=True)):
        with pytest.raises(ValueError):
            cv_hip.solvePnPTagConsensus(obj, img, sc.K, sc.dist, **kw)
    with pytest.raises(ValueError):
        cv_hip.solvePnPTagConsensus(obj[:46], img[:46], sc.K, sc.dist)
    with pytest.raises(ValueError):
        cv_hip.solvePnPTagConsensus(np.zeros((260, 3), np.float32), np.zeros((260, 2), np.float32), sc.K, sc.dist)
    Det = _detector_class(tmp_path, sc, "args")
    for bad in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            Det(LOG, sc.K, sc.dist, True, pnp_consensus_px=bad)
    from accurate_aprilgroup_tracking_amd.pose_detector import tag_consensus
    with pytest.raises(ValueError):
        tag_consensus(None, obj, img, sc.K, sc.dist, inlier_px=0.0)
    with pytest.raises(ValueError):
        tag_consensus(None, obj[:46], img[:46], sc.K, sc.dist)


def _detector_class(tmp_path, sc, tag):
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    d = tmp_path / ("g_%s" % tag)
    d.mkdir(exist_ok=True)
    (d / "april_group.json").write_text(json.dumps(sc.group))

    class Det(PoseDetector):
        DIRPATH = str(d)
    return Det


def _lists(sc, img):
    return [img[4 * t:4 * t + 4].reshape(1, 4, 2).astype(np.float64) for t in range(sc.n_tags)], [sc.obj[4 * t:4 * t + 4] for t in range(sc.n_tags)]


CASES = [(nb, seed, guess) for nb in (0, 3, 5) for seed in (0, 1, 2) for guess in (False, True)]


@pytest.mark.parametrize("n_bad,seed,guess", CASES)
def test_host_rule_is_the_numpy_statement_and_recovers_the_clean_corners(oracle, tmp_path, n_bad, seed, guess):
    """The 18 cases: 12 tags, 640 x 480, five lens coefficients, 0.05 px noise, 0 / 3 / 5 whole tags displaced by 6 - 25 px, seeds 0 - 2,
    with and without a guess.  PoseDetector(backend="cv", cv=oracle, pnp_consensus_px=2) elects what rule() elects -- exactly the
    undisplaced corners -- and its pose is the refit's; without the option the same input fails the 2 px gate whenever a tag is displaced."""
    from oracle import cv2_shim
    from accurate_aprilgroup_tracking_amd.pose_detector import tag_consensus
    sc = S.Scene(12, seed, n_bad)
    img = sc.img()
    g = sc.guess if guess else None
    res = S.oracle_rule(oracle, sc.obj, img, sc.K, sc.dist, guess=g)
    closest = S.check_margins(res, np.ones(sc.n, bool))
    print("closest residual to the threshold %.3f px; per-tag counts %s" % (closest, sorted(set(res["counts"].values()))))
    assert np.array_equal(res["inliers"], sc.clean) and res["count"] == int(sc.clean.sum()) and res["n_hyp"] == 12
    assert sorted(set(res["counts"].values())) == ([4, res["count"]] if n_bad else [48])
    # the host rule, as a function ...
    cv = cv2_shim.make_cv2()
    inl, win, cnt, pose = tag_consensus(cv, sc.obj, img, sc.K, sc.dist, guess=None if g is None else (g[:3].reshape(3, 1), g[3:].reshape(3, 1)))
    assert np.array_equal(inl, res["inliers"]) and (win, cnt) == (res["winner"], res["count"])
    assert np.array_equal(np.concatenate([pose[0].ravel(), pose[1].ravel()]), res["pose"])
    # ... and inside the state machine
    Det = _detector_class(tmp_path, sc, "h%d%d%d" % (n_bad, seed, guess))
    det = Det(LOG, sc.K, sc.dist, True, cv=cv, pnp_consensus_px=S.TAU)
    plain = Det(LOG, sc.K, sc.dist, True, cv=cv)
    il, ol = _lists(sc, img)
    for d in (det, plain):
        if guess:
            d.extrinsic_guess = (g[:3].copy().reshape(3, 1), g[3:].copy().reshape(3, 1))
            d.prev_transform = (sc.rvec.copy().reshape(3, 1) + 0.02, sc.tvec.copy().reshape(3, 1))
        d._estimate_pose(list(il), list(ol))
    assert det.last_consensus == (res["winner"], res["count"])
    # the refit of the rule starts from the winner's pose; the state machine's solve from its own guess: same minimum, not the same bits
    refit, _ = S.oracle_refit(oracle, sc.obj, img, sc.K, sc.dist, res)
    got = np.concatenate([det.last_pose[0].ravel(), det.last_pose[1].ravel()]).astype(np.float64)
    assert np.abs(got[:3] - refit[:3]).max() < 1e-5 and np.abs(got[3:] - refit[3:]).max() < 1e-5
    assert det.last_error < 0.2 and np.abs(refit[:3] - sc.rvec).max() < 2e-3
    if n_bad:
        assert plain.last_error > 2.0, "the plain solve passes the gate with %d displaced tags (%.2f px)" % (n_bad, plain.last_error)
        assert np.abs(np.asarray(plain.last_pose[0], np.float64).ravel() - sc.rvec).max() > 10 * np.abs(refit[:3] - sc.rvec).max()
    else:
        assert plain.last_error < 0.2


@pytest.mark.parametrize("kind", S.BATCHES + S.EDGE_BATCHES)
def test_every_gpu_batch_meets_the_margin_condition(oracle, kind):
    """(e_flag is exempt from nothing either: with its reference told what the zero tag reports, it meets the condition too)"""
    bt = S.make_batch(kind, oracle)
    for b in range(bt.B):
        for guess in (False, True):
            res = bt.reference(oracle, b, guess)
            S.check_margins(res, bt.usable(b))
            assert np.array_equal(res["inliers"], bt.expected[b]), "%s stream %d" % (kind, b)
            if kind == "b2_allbad" and b == 1:
                assert res["winner"] == -1 and res["n_hyp"] == 12 and max(res["counts"].values()) == 4
            if kind.endswith("masked"):
                assert res["n_cand"] == 11 and res["count"] == int(bt.expected[b].sum()) and res["count"] % 4 == 3


# what the oracle's rule gives for every edge batch: (n_cand, n_hyp without a guess, n_hyp with one, winner per stream, count)
EDGE_TABLE = {"e_nonfinite": (12, 10, 10, (8,), 34), "e_noncoplanar": (12, 11, 12, (8,), 36), "e_tie": (12, 12, 12, (5,), 8),
              "e_behind": (10, 10, 10, (1,), 32), "e_t64": (64, 64, 64, (S.E_T64_WINNER,), 176), "e_t64_last": (64, 64, 64, (63,), 176),
              "e_t1": (1, 1, 1, (0,), 4), "e_cpt8": (6, 6, 6, (4,), 40), "e_cpt80": (3, 3, 3, (1, 0), 160), "e_cpt128": (1, 1, 1, (0,), 255),
              "e_flag": (12, 11, 11, (8,), 44)}


@pytest.mark.parametrize("kind", S.EDGE_BATCHES)
def test_edge_batches_reach_their_clause(oracle, kind):
    """The edge batches of the GPU tests, by the oracle alone: candidates, accepted hypotheses, winner and count are the table's, and each
    scene's outcome hangs on the clause it was built for."""
    bt = S.make_batch(kind, oracle)
    n_cand, hyp_plain, hyp_guess, winners, count = EDGE_TABLE[kind]
    for b in range(bt.B):
        for guess in (False, True):
            res = bt.reference(oracle, b, guess)
            where = "%s stream %d %s" % (kind, b, "guess" if guess else "no guess")
            assert (res["n_cand"], res["n_hyp"]) == (n_cand, hyp_guess if guess else hyp_plain), where
            assert (res["winner"], res["count"]) == (winners[b], count) and count == int(bt.expected[b].sum()), where
            assert np.array_equal(res["inliers"], bt.expected[b]), where
            if kind == "e_nonfinite":
                bad = np.flatnonzero(~np.isfinite(bt.img[b]).all(axis=1))
                assert bad.size == 2 and bt.usable(b)[bad].all() and not res["inliers"][bad].any(), where
                assert sorted(set(range(12)) - set(res["counts"])) == sorted(bad // 4), where + ": the two tags are no hypotheses"
            if kind == "e_tie":
                assert res["counts"] == {t: (8 if t in (5, 9) else 4) for t in range(12)}, where
                assert res["ssq"][5] == res["ssq"][9] and np.array_equal(res["sets"][5], res["sets"][9]), where + ": an exact tie"
                assert count == bt.min_inliers, where + ": the count sits on min_inliers"
                none = S.oracle_rule(oracle, bt.obj, bt.img[b], bt.K, bt.dist, guess=bt.guess[b] if guess else None, min_inliers=9)
                assert none["winner"] == -1 and not none["inliers"].any(), where
            if kind == "e_behind":
                twins = np.flatnonzero(bt.mask[b] == 0) // 4
                tw = np.concatenate([np.arange(4 * d + 1, 4 * d + 4) for d in twins])
                d = np.sqrt(res["d2"][res["winner"]][tw])
                print("%s: the twins' usable corners lie %.2f .. %.2f px from their image points under the winner" % (where, d.min(), d.max()))
                assert twins.size == 2 and d.max() < S.TAU - 0.05 and not res["inliers"][tw].any(), where
                # ... and nothing but the depth clause keeps them out
                wo = bt.reference(oracle, b, guess, depth_clause=False)
                assert wo["count"] == count + 6 and wo["inliers"][tw].all() and np.array_equal(wo["inliers"][bt.expected[b]], res["inliers"][bt.expected[b]]), where
            if kind == "e_flag":
                t = S.E_FLAG_TAG
                assert t not in res["counts"], where
                if guess:
                    # without the flag clause the zero tag's hypothesis, the guess itself, beats every tag's
                    wo = bt.reference(oracle, b, guess, flag_clause=False)
                    assert wo["winner"] == t and wo["n_hyp"] == 12 and wo["count"] == count, where
            if kind.startswith("e_cpt"):
                assert set(res["counts"].values()) <= {bt.cpt, count}, where


def test_option_off_is_the_detector_without_the_keyword(oracle, tmp_path):
    from oracle import cv2_shim
    sc = S.Scene(12, 1, 3)
    cv = cv2_shim.make_cv2()
    Det = _detector_class(tmp_path, sc, "off")
    il, ol = _lists(sc, sc.img())
    out = []
    for kw in ({}, dict(pnp_consensus_px=None), dict(pnp_consensus_px=0)):
        d = Det(LOG, sc.K, sc.dist, True, cv=cv, **kw)
        assert d.pnp_consensus_px is None
        for _ in range(2):
            d._estimate_pose(list(il), list(ol))
        out.append((np.concatenate([d.last_pose[0].ravel(), d.last_pose[1].ravel()]), d.last_error, d.extrinsic_guess[0] is None))
    for o in out[1:]:
        assert np.array_equal(o[0], out[0][0]) and o[1] == out[0][1] and o[2] == out[0][2]


def test_rule_edge_cases():
    """NaN residuals vote for nobody, points behind the camera are no inliers, ties go to the smaller sum of squares, then the lower tag"""
    obj = np.zeros((8, 3), np.float32)
    img = np.zeros((8, 2), np.float32)
    img[4:] = 10.0
    poses = {0: np.array([0, 0, 0, 0, 0, 1.0]), 1: np.array([0, 0, 0, 0, 0, 1.0])}
    proj = {0: np.zeros((8, 2)), 1: np.full((8, 2), 10.0)}
    key = lambda p: 0 if p is poses[0] else 1
    res = S.rule(obj, img, np.ones(8, bool), lambda t: (poses[t], 0), lambda p: proj[key(p)], min_inliers=4)
    assert res["winner"] == 0 and res["count"] == 4 and res["counts"] == {0: 4, 1: 4}            # exact tie: the lower tag
    proj[0] = np.full((8, 2), 0.1)
    res = S.rule(obj, img, np.ones(8, bool), lambda t: (poses[t], 0), lambda p: proj[key(p)], min_inliers=4)
    assert res["winner"] == 1                                                                       # smaller sum of squares
    proj[1] = np.full((8, 2), np.nan)
    res = S.rule(obj, img, np.ones(8, bool), lambda t: (poses[t], 0), lambda p: proj[key(p)], min_inliers=4)
    assert res["winner"] == 0 and res["counts"][1] == 0
    poses[0] = np.array([0, 0, 0, 0, 0, -1.0])
    res = S.rule(obj, img, np.ones(8, bool), lambda t: (poses[t], 0), lambda p: proj[key(p)], min_inliers=4)
    assert res["winner"] == -1 and not res["inliers"].any() and res["counts"] == {0: 0, 1: 0}
    res = S.rule(obj, img, np.ones(8, bool), lambda t: (poses[t], S.TOO_FEW if t else S.SINGULAR), lambda p: proj[key(p)], min_inliers=4)
    assert res["n_cand"] == 2 and res["n_hyp"] == 0 and res["winner"] == -1


def test_tracker_scene_does_its_work_on_the_cpu(oracle, tmp_path):
    """the sliding-tags scene of the GPU tracker tests, by the mirror alone: every frame's vote meets the margin condition (asserted inside
    mirror_chain), the mirror accepts every frame with the option on and rejects the covered frames with it off"""
    sc = S.SlidingSequence()
    on = S.mirror_chain(oracle, sc, tmp_path, "on", S.TAU)
    off = S.mirror_chain(oracle, sc, tmp_path, "off", None)
    print("with the option: err %s consensus %s margins %s; without: err %s" % ([r["err"] for r in on], [r["consensus"] for r in on],
                                                                               [r["closest"] for r in on], [r["err"] for r in off]))
    assert all(r["ok"] for r in on) and all(r["status"].all() for r in on)
    assert [r["ok"] for r in off] == [k < S.OCC_FROM for k in range(1, len(sc))]
    assert all(r["consensus"][1] < 48 for r in on[S.OCC_FROM - 1:]) and on[0]["consensus"][1] == 48
    # the one-frame compositions of the GPU test start at frame OCC_FROM - 1
    for fb in (None, 1.0):
        r = S.mirror_chain(oracle, sc, tmp_path, "one%s" % fb, S.TAU, k0=S.OCC_FROM - 1, steps=1, fb_px=fb)[0]
        assert r["ok"] and r["consensus"][1] == 40
