"""CPU: the dense-model library (include/agt_model.h -> libagt_model.so) builds, exports exactly its header and keeps its kernels out
of scratch; the numpy statement of the accumulation rule (tests/dense_model_numpy.py) that the GPU tests compare with equals a plain
per-observation loop; the scenes (tests/dense_model_scenes.py) meet the conditions the GPU tests rely on; lattice and file format."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import calib_scenes                # noqa: E402
import dense_model_numpy as dm     # noqa: E402
import dense_model_scenes as sc    # noqa: E402
import pnp_numpy                   # noqa: E402

from accurate_aprilgroup_tracking_amd import synthetic     # noqa: E402

KERNELS = ["model_accumulate_kernel", "model_frames_kernel"]
CAMERAS = {"none": None, "mild": synthetic.MILD_DIST.reshape(-1), "tilt14": calib_scenes.TILT14}


def test_model_library_builds_exports_and_resources():
    import side_library
    from accurate_aprilgroup_tracking_amd import modellib
    rows = side_library.built(modellib, "model")
    assert sorted(re.search(r"(model_\w+)\(", r["name"]).group(1) for r in rows) == KERNELS
    bad = [(r["name"], r["scratch"], r["vgpr"], r["vspill"]) for r in rows if r["scratch"] != 0 or r["vgpr"] > 512 or r["vspill"] != 0]
    assert not bad, bad
    L = modellib.lib()
    assert L.agt_model_version() == modellib.VERSION == 100
    # argument errors are judged before any device work
    h = ctypes.c_void_p()
    assert L.agt_dense_model_create(None, None, ctypes.byref(h)) == modellib.ERR_ARG
    K = np.eye(3); tc = np.zeros((257, 4, 3), np.float32); xyz = np.zeros((1, 3), np.float32); tag = np.zeros(1, np.int32)
    p = modellib.Problem(K.ctypes.data, None, 0, 64, 64, 257, tc.ctypes.data, 1, 1, xyz.ctypes.data, tag.ctypes.data, 60.0)
    assert L.agt_dense_model_create(ctypes.byref(p), None, ctypes.byref(h)) == modellib.ERR_ARG and not h.value
    p.n_tags = 1; p.ndist = 3
    assert L.agt_dense_model_create(ctypes.byref(p), None, ctypes.byref(h)) == modellib.ERR_CAMERA and not h.value
    assert L.agt_dense_model_destroy(None) == 0
    assert L.agt_dense_model_begin_pass(None, 0.0, 0.0) == modellib.ERR_ARG
    assert L.agt_dense_model_read(None, None, None, None, None) == modellib.ERR_ARG


def test_missing_library_raises(monkeypatch):
    from accurate_aprilgroup_tracking_amd import modellib
    monkeypatch.setattr(modellib, "_lib", None)
    monkeypatch.setattr(modellib, "LIB_PATH", "/nonexistent/libagt_model.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        modellib.lib()


def loop_pass(prob, frames, poses, use, ref, clip_sigma, sigma_floor):
    """the rule of include/agt_model.h, one observation at a time in plain Python floats"""
    n, rej = [0] * prob.M, [0] * prob.M
    S, S2 = [0.0] * prob.M, [0.0] * prob.M
    fobs = [0] * len(poses)
    cos_max = 0.0 if prob.max_view_deg == 90.0 else math.cos(math.radians(prob.max_view_deg))
    for f, pose in enumerate(poses):
        if use is not None and not use[f]:
            continue
        R, _ = pnp_numpy.rodrigues(pose[:3])
        t = pose[3:]
        vis = []
        for c in prob.corners:
            co = (((c[0] + c[1]) + c[2]) + c[3]) * 0.25
            no = prob.facing * np.cross(c[3] - c[0], c[1] - c[0])
            cc, nc = R @ co + t, R @ no
            cos = -float(nc @ cc) / (math.sqrt(float(nc @ nc)) * math.sqrt(float(cc @ cc)))
            vis.append(cc[2] > 0 and cos > cos_max)
        img = frames[f]
        for i in range(prob.M):
            if not vis[prob.tag[i]] or (R @ prob.X[i] + t)[2] <= 0:
                continue
            u, v = pnp_numpy.project(prob.X[i:i + 1], pose[:3], pose[3:], prob.K, prob.dist)[0]
            x0, y0 = math.floor(u), math.floor(v)
            if not (1 <= x0 <= prob.w - 3 and 1 <= y0 <= prob.h - 3):
                continue
            a, b = u - x0, v - y0
            I = (1 - a) * (1 - b) * float(img[y0, x0]) + a * (1 - b) * float(img[y0, x0 + 1]) + (1 - a) * b * float(img[y0 + 1, x0]) \
                + a * b * float(img[y0 + 1, x0 + 1])
            if clip_sigma > 0 and ref["n"][i] > 0:
                mean = ref["S"][i] / ref["n"][i]
                std = math.sqrt(max(ref["S2"][i] / ref["n"][i] - mean * mean, 0.0))
                if abs(I - mean) > clip_sigma * max(std, sigma_floor):
                    rej[i] += 1
                    continue
            n[i] += 1; S[i] += I; S2[i] += I * I; fobs[f] += 1
    return dict(n=np.array(n), S=np.array(S), S2=np.array(S2), rejected=np.array(rej), frame_obs=np.array(fobs))


@pytest.mark.parametrize("camera", ["none", "tilt14"])
def test_statement_equals_a_plain_loop(camera):
    s = sc.rotating().with_camera(CAMERAS[camera])
    sel = np.flatnonzero(np.isin(s.tag, (0, 3, 7)))                    # a 3-tag scene: 75 samples
    prob = s.problem(sel)
    use = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1], np.uint8)
    plain, clipped = dm.learn(prob, s.frames, s.poses, use, 1.5, 4.0)
    lp = loop_pass(prob, s.frames, s.poses, use, None, 0.0, 0.0)
    lc = loop_pass(prob, s.frames, s.poses, use, lp, 1.5, 4.0)
    assert plain["n"].sum() > 150 and clipped["rejected"].sum() > 0 and (plain["n"] == 0).sum() == 0
    for a, b in ((plain, lp), (clipped, lc)):
        for k in ("n", "rejected", "frame_obs"):
            assert np.array_equal(a[k], b[k]), k
        assert np.abs(a["S"] - b["S"]).max() < 1e-9 and np.abs(a["S2"] - b["S2"]).max() < 1e-6


def scene_cases():
    return [(name, cam) for name in ("rotating", "border", "clean640") for cam in CAMERAS] + [("occluder", "none")]


@pytest.mark.parametrize("name,camera", scene_cases())
def test_scene_conditions(name, camera):
    """a scene in which a decision of the rule is nearly a tie is not a scene"""
    s = getattr(sc, name)().with_camera(CAMERAS[camera])
    plain, final = dm.learn(s.problem(), s.frames, s.poses)
    m = final["margins"]
    print("%s / %s: margins cos %.3g window %.3g px clip %.3g; observations %d, rejected %d" %
          (name, camera, m["cos"], m["window"], m["clip"], final["n"].sum(), final["rejected"].sum()))
    assert m["cos"] >= 1e-3 and m["window"] >= 1e-4 and m["clip"] >= 1e-6 and dm.margins_ok(m)
    assert plain["margins"]["cos"] == m["cos"] and plain["margins"]["window"] == m["window"]
    if name == "rotating":
        vis = np.array([dm.tag_visibility(s.problem(), p)[0] for p in s.poses])
        assert ((vis.sum(axis=0) > 0) & (vis.sum(axis=0) < len(s.poses))).all(), "every tag flips, none stays unseen"
        assert s.xyz.shape[0] == 300
    if name == "border":
        obs = plain["frame_obs"]
        assert (np.diff(obs) < 0).all() and obs[0] > 3 * obs[-1] > 0, obs


def test_occluder_is_clipped_on_the_statement():
    clean, occ = sc.clean640(), sc.occluder()
    pc, fc = dm.learn(clean.problem(), clean.frames, clean.poses)
    po, fo = dm.learn(occ.problem(), occ.frames, occ.poses)
    k = occ.tag == sc.OCCLUDED_TAG
    tc, tp, tf = dm.template(pc)[k], dm.template(po)[k], dm.template(fo)[k]
    ok = np.isfinite(tc) & np.isfinite(tp) & np.isfinite(tf)
    assert ok.sum() == 64
    rms_plain, rms_clipped = np.sqrt(np.mean((tp - tc)[ok] ** 2)), np.sqrt(np.mean((tf - tc)[ok] ** 2))
    frac = fc["rejected"].sum() / (fc["rejected"].sum() + fc["n"].sum())
    print("tag %d vs the clean template: plain %.3g, clipped %.3g gray levels RMS; clean frames reject %.1f %%" %
          (sc.OCCLUDED_TAG, rms_plain, rms_clipped, 100 * frac))
    assert rms_clipped <= 0.25 * rms_plain
    assert frac <= 0.10


def test_lattice_is_model_samples_bitwise():
    from accurate_aprilgroup_tracking_amd import dense_model
    for n_tags, grid in ((12, 5), (3, 32), (60, 4)):
        group = synthetic.make_april_group(n_tags=n_tags, seed=n_tags)
        xyz, tag, corners = dense_model.lattice(group, grid)
        assert xyz.dtype == np.float32 and tag.dtype == np.int32 and corners.dtype == np.float32
        assert np.array_equal(xyz.view(np.uint32), synthetic.model_samples(group, grid).view(np.uint32))
        assert np.array_equal(tag, np.repeat(np.arange(n_tags), grid * grid))
        assert np.array_equal(corners.reshape(-1, 3), synthetic.group_object_points(group).astype(np.float32))
        # the loader's form of the same group gives the same lattice
        ext = {int(k): [v["size"], np.array(v["extrinsics"][:3], np.float32).reshape(3, 1), np.array(v["extrinsics"][-3:], np.float32).reshape(3, 1)]
               for k, v in group["tags"].items()}
        x2, t2, c2 = dense_model.lattice(ext, grid)
        assert np.array_equal(x2.view(np.uint32), xyz.view(np.uint32)) and np.array_equal(t2, tag) and np.array_equal(c2, corners)


def test_statistics():
    from accurate_aprilgroup_tracking_amd import dense_model
    mean, std = dense_model.statistics([0, 1, 4], [0.0, 7.0, 10.0], [0.0, 49.0, 30.0])
    assert np.isnan(mean[0]) and np.isnan(std[0]) and mean[1] == 7.0 and std[1] == 0.0 and mean[2] == 2.5 and std[2] == math.sqrt(30 / 4 - 6.25)


def test_dense_model_format_round_trip(tmp_path):
    from accurate_aprilgroup_tracking_amd import dense_model, formats
    rng = np.random.default_rng(0)
    xyz, tag, _ = dense_model.lattice(synthetic.make_april_group(n_tags=3), 4)
    M = xyz.shape[0]
    n = rng.integers(0, 9, M).astype(np.int32)
    model = dense_model.DenseModel(xyz, (rng.random(M) * 255).astype(np.float32), tag, n, rng.random(M) * 1e-3 + 1e-9, rng.integers(0, 3, M), n >= 4,
                                   rng.integers(0, 99, 7), dict(grid=4, extent=0.6, max_view_deg=60.0, facing=1, clip_sigma=1.5, max_std=float("inf")))
    path = tmp_path / "model.npz"
    formats.save_dense_model(path, model)
    back = formats.load_dense_model(path)
    for k in dense_model.DenseModel.FIELDS:
        a, b = getattr(model, k), getattr(back, k)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert back.settings == model.settings and type(back.settings["grid"]) is int
    with np.load(path, allow_pickle=False) as f:                   # arrays and plain settings only
        assert all(f[k].dtype.kind in "fiub" for k in f.files)
    c = back.compact()
    assert c.model_xyz.shape[0] == int((n >= 4).sum()) and c.usable.all() and np.array_equal(c.model_t, model.model_t[n >= 4])
    assert "usable" in back.report()
    np.savez(tmp_path / "bad.npz", model_xyz=xyz)
    with pytest.raises(ValueError, match="missing"):
        formats.load_dense_model(tmp_path / "bad.npz")
