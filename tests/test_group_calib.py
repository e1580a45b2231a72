"""CPU: the calibration library (include/agt_calib.h -> libagt_calib.so) builds, exports exactly its header and keeps its kernels out
of scratch; the numpy / scipy statement of the bundle adjustment (tests/group_ba_numpy.py) that the GPU tests compare with is sound
(recovers the truth, Schur step = dense step); the scene builders give what the GPU tests assume."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import calib_scenes as cs          # noqa: E402
import group_ba_numpy as ba        # noqa: E402
import pnp_numpy                   # noqa: E402

KERNELS = ["calib_accumulate_kernel", "calib_backsub_kernel", "calib_cost_kernel", "calib_eliminate_kernel", "calib_reduce_kernel"]
E2E_PERTURB_DEG = cs.E2E_PERTURB_DEG


def test_calib_library_builds_exports_and_resources():
    import side_library
    from accurate_aprilgroup_tracking_amd import caliblib
    rows = side_library.built(caliblib, "calib")
    assert [re.search(r"(calib_\w+)\(", r["name"]).group(1) for r in rows] == KERNELS
    bad = [(r["name"], r["scratch"], r["vgpr"], r["vspill"]) for r in rows if r["scratch"] != 0 or r["vgpr"] > 512 or r["vspill"] != 0]
    assert not bad, bad
    L = caliblib.lib()
    assert L.agt_calib_version() == caliblib.VERSION == 100
    # argument errors are judged before any device work
    h = ctypes.c_void_p()
    assert L.agt_group_calib_create(None, None, ctypes.byref(h)) == caliblib.ERR_ARG
    sizes = np.full(65, 0.02); K = np.eye(3)
    p = caliblib.Problem(K.ctypes.data, None, 0, 65, sizes.ctypes.data, 0, 4, 0, 0, None, None, None)
    assert L.agt_group_calib_create(ctypes.byref(p), None, ctypes.byref(h)) == caliblib.ERR_ARG and not h.value
    assert L.agt_group_calib_destroy(None) == 0


def test_missing_library_raises(monkeypatch):
    from accurate_aprilgroup_tracking_amd import caliblib
    monkeypatch.setattr(caliblib, "_lib", None)
    monkeypatch.setattr(caliblib, "LIB_PATH", "/nonexistent/libagt_calib.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        caliblib.lib()


def test_scene_builders():
    for sc, want in [(cs.parity_scene(), [1, 5, 2, 3, 2, 2, 3]), (cs.wave_scene(), [2, 3, 2, 3, 17, 3, 2, 3, 2]), (cs.smallest_scene(), [2, 2, 2])]:
        assert sc.visible.sum(axis=1).tolist() == want and sc.connected(0)
    assert cs.parity_scene().visible[:, 4].sum() == 2
    # the flat board: every tag in every frame, rotation vectors exactly 0 in the truth and in the start, the anchor (tag 4) the origin
    sc = cs.flat_board_scene()
    tp, fp = cs.flat_start(sc)
    assert sc.visible.all() and sc.connected(cs.FLAT_ANCHOR) and not tp[:, :3].any() and not tp[cs.FLAT_ANCHOR].any()
    assert np.abs(ba.residuals(sc.problem(cs.FLAT_ANCHOR), sc.tag_poses, sc.frame_poses)).max() < 1e-9
    assert 0.1 < np.abs(ba.residuals(sc.problem(cs.FLAT_ANCHOR), tp, fp)).max() < 20.0
    for sc in (cs.recovery_scene(), cs.noisy_scene(48)):
        assert sc.connected(0)
        assert (sc.visible.sum(axis=1) >= 2).mean() > 0.9 and sc.visible.any(axis=0).all()
        # the facing test did hide tags: no frame sees the whole group
        assert (sc.visible.sum(axis=1) < len(sc.tag_ids)).all()
    # the truth explains a noise-free scene to round-off, in the group's frame and in the anchor's
    sc = cs.recovery_scene()
    assert np.abs(ba.residuals(sc.problem(0), sc.tag_poses, sc.frame_poses)).max() < 1e-9
    tp, fp = sc.in_anchor_frame(2)
    assert np.abs(tp[2]).max() < 1e-12 and np.abs(ba.residuals(sc.problem(2), tp, fp)).max() < 1e-9


def test_numpy_reference_recovers_the_truth():
    sc = cs.recovery_scene()
    prob = sc.problem(0)
    tag0, frame0 = cs.perturbed_start(sc, frames=False)
    tp, fp, cost, rms = ba.solve(prob, tag0, frame0)
    print("scipy vs truth: tags %.3g frames %.3g rms %.3g" % (np.abs(tp - sc.tag_poses).max(), np.abs(fp - sc.frame_poses).max(), rms))
    assert np.abs(tp - sc.tag_poses).max() < 1e-10 and np.abs(fp - sc.frame_poses).max() < 1e-10 and rms < 1e-10
    assert np.array_equal(tp[0], sc.tag_poses[0])          # the anchor is fixed


def test_numpy_jacobian_is_the_derivative():
    sc = cs.parity_scene(cs.TILT14)
    prob = sc.problem(1)
    rng = np.random.default_rng(2)
    tp = sc.tag_poses + 1e-2 * rng.standard_normal(sc.tag_poses.shape)
    fp = sc.frame_poses + 1e-2 * rng.standard_normal(sc.frame_poses.shape)
    _, J = ba.jacobian(prob, tp, fp)
    fc, tc, m = ba.layout(prob)
    for cols, arr in ((fc, fp), (tc, tp)):
        for idx, c in cols.items():
            for j in range(6):
                h = 1e-6
                a, b = arr.copy(), arr.copy()
                a[idx, j] += h; b[idx, j] -= h
                args = (lambda x: (tp, x)) if arr is fp else (lambda x: (x, fp))
                num = (ba.residuals(prob, *args(a)) - ba.residuals(prob, *args(b))).ravel() / (2 * h)
                assert np.abs(num - J[:, c + j]).max() < 1e-4 * max(1.0, np.abs(J[:, c + j]).max())


@pytest.mark.parametrize("name", ["parity", "tilt", "wave", "smallest", "flat"])
def test_numpy_schur_step_equals_dense_step(name):
    """the difference measured here is the floor of the GPU step tolerance (tests/test_gpu_group_calib.py)"""
    sc = {"parity": cs.parity_scene, "tilt": lambda: cs.parity_scene(cs.TILT14), "wave": cs.wave_scene, "smallest": cs.smallest_scene,
          "flat": cs.flat_board_scene}[name]()
    prob = sc.problem(cs.FLAT_ANCHOR if name == "flat" else 0)
    tp, fp = cs.flat_start(sc) if name == "flat" else cs.perturbed_start(sc)
    for lam in (0.0, 1e-3, 10.0):
        d = ba.step_difference(ba.schur_step(prob, tp, fp, lam), ba.dense_step(prob, tp, fp, lam))
        print("%s lambda %g: |schur - dense| / |dense| = %.3g" % (name, lam, d))
        assert d < 1e-8


def test_group_json_round_trip(tmp_path):
    from accurate_aprilgroup_tracking_amd import formats, group_calib, synthetic
    sc = cs.recovery_scene()
    poses = sc.tag_poses + 1e-9          # not float32-representable
    group = group_calib.poses_to_group(poses, sc.tag_ids, sc.sizes)
    formats.save_april_group(tmp_path / "a.json", group)
    synthetic.write_april_group(tmp_path / "b.json", group)
    for name in ("a.json", "b.json"):
        back = formats.load_april_group(tmp_path / name)
        assert sorted(back) == sc.tag_ids
        for i, t in enumerate(sc.tag_ids):
            assert back[t][0] == sc.sizes[i]
            assert np.array_equal(back[t][1].ravel(), poses[i, 3:].astype(np.float32)) and np.array_equal(back[t][2].ravel(), poses[i, :3].astype(np.float32))
    assert np.array_equal(group_calib.group_to_poses(group, sc.tag_ids), poses.astype(np.float32).astype(np.float64))
    assert np.array_equal(group_calib.group_to_poses(formats.load_april_group(tmp_path / "a.json"), sc.tag_ids), poses.astype(np.float32).astype(np.float64))


def test_observation_table_filters():
    from accurate_aprilgroup_tracking_amd import formats, group_calib
    c = np.arange(8.0).reshape(4, 2)
    frames = [[formats.make_detection(3, c), formats.make_detection(5, c + 1, decision_margin=10.0), formats.make_detection(9, c)],
              [], [formats.make_detection(5, c + 2), formats.make_detection(5, c + 3)]]
    fr, tg, co = group_calib.observation_table(frames, [3, 5])
    assert fr.tolist() == [0, 2] and tg.tolist() == [0, 1] and np.array_equal(co[1], c + 3)


def test_nominal_model_fails_the_gate():
    """the premise of the end-to-end GPU test, confirmed with the numpy solvePnP: a model whose tags sit E2E_PERTURB_DEG off fails the
    2 px gate (mean corner error of the solved pose) on at least one frame of the clip, the true model on none"""
    from accurate_aprilgroup_tracking_amd import group_calib
    sc = cs.e2e_scene()
    worst = {}
    for name, poses in (("truth", sc.tag_poses), ("nominal", cs.e2e_nominal(sc))):
        obj = group_calib.object_points(poses, sc.sizes).reshape(-1, 4, 3)
        errs = []
        for f, dets in enumerate(sc.frames):
            idx = [sc.tag_ids.index(d.tag_id) for d in dets]
            o = obj[idx].reshape(-1, 3); img = np.concatenate([d.corners for d in dets])
            r, t, _ = pnp_numpy.solve_pnp_guess(o, img, sc.K, sc.dist, sc.frame_poses[f, :3], sc.frame_poses[f, 3:])
            errs.append(np.linalg.norm(pnp_numpy.project(o, r, t, sc.K, sc.dist) - img, axis=1).mean())
        worst[name] = max(errs)
    print("worst mean reprojection error: truth %.3g px, nominal %.3g px" % (worst["truth"], worst["nominal"]))
    assert worst["truth"] < 1e-3 and worst["nominal"] > 2.0
