"""GPU: libagt_model.so (include/agt_model.h) against the numpy statement of its rule (tests/dense_model_numpy.py) on the scenes of
tests/dense_model_scenes.py -- whose decisions are nowhere near a tie (tests/test_dense_model.py::test_scene_conditions).

Parity bounds: n, rejected and frame_obs are equal exactly; |S / n - statement| <= 1e-9 and |S2 / n - statement| <= 1e-6.  Pixel
coordinates of the device projection and of the numpy one agree to ~1e-13 px (profiles/group_calib.md); the image gradient is at most
255 per px, so one observation differs by <= 3e-11 and its square by <= 1.5e-8: the bounds leave about 30x.  The measured maxima are
printed (profiles/dense_model.md holds them).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import calib_scenes                # noqa: E402
import dense_model_numpy as dm     # noqa: E402
import dense_model_scenes as sc    # noqa: E402
import dense_numpy                 # noqa: E402
import pnp_numpy                   # noqa: E402

from accurate_aprilgroup_tracking_amd import synthetic     # noqa: E402

pytestmark = pytest.mark.gpu

CAMERAS = {"none": None, "mild": synthetic.MILD_DIST.reshape(-1), "tilt14": calib_scenes.TILT14}
S_BOUND, S2_BOUND = 1e-9, 1e-6
CLIP = (1.5, 4.0)

_statement = {}


def scene_of(name, camera="none"):
    return getattr(sc, name)().with_camera(CAMERAS[camera])


def statement(name, camera="none"):
    """(plain, clipped) of the whole scene by the statement: computed once, shared, never changed"""
    if (name, camera) not in _statement:
        s = scene_of(name, camera)
        plain, clipped = dm.learn(s.problem(), s.frames, s.poses, None, *CLIP)
        for r in (plain, clipped):
            assert dm.margins_ok(r["margins"]), r["margins"]
            for a in r.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _statement[(name, camera)] = (plain, clipped)
    return _statement[(name, camera)]


def builder(s, sel=None):
    from accurate_aprilgroup_tracking_amd import dense_model
    xyz, tag = (s.xyz, s.tag) if sel is None else (s.xyz[sel], s.tag[sel])
    return dense_model.DenseModelBuilder(s.K, s.dist, s.width, s.height, s.corners, xyz, tag, s.max_view_deg, 1)


def run_library(b, frames, poses, use=None, cuts=None, clip=None):
    """one pass (the builder's next one) over `frames` cut into calls at `cuts` -> dict like the statement's"""
    b.begin_pass(*(clip or (0.0, 0.0)))
    edges = [0] + list(cuts or []) + [len(frames)]
    obs = [b.accumulate(frames[a:z], poses[a:z], None if use is None else use[a:z]) for a, z in zip(edges[:-1], edges[1:])]
    n, S, S2, rej = b.read()
    return dict(n=n, S=S, S2=S2, rejected=rej, frame_obs=np.concatenate(obs))


def parity(lib, ref, label):
    assert np.array_equal(lib["n"], ref["n"]), label + ": n"
    assert np.array_equal(lib["rejected"], ref["rejected"]), label + ": rejected"
    assert np.array_equal(lib["frame_obs"], ref["frame_obs"]), label + ": frame_obs"
    k = ref["n"] > 0
    nn = np.where(k, ref["n"], 1)
    dS = float(np.abs(lib["S"] / nn - ref["S"] / nn).max())
    dS2 = float(np.abs(lib["S2"] / nn - ref["S2"] / nn).max())
    print("%s: %d observations, %d rejected; max |S/n - statement| %.3g, max |S2/n - statement| %.3g" %
          (label, int(ref["n"].sum()), int(ref["rejected"].sum()), dS, dS2))
    assert (lib["S"][~k] == 0).all() and (lib["S2"][~k] == 0).all()
    assert dS <= S_BOUND and dS2 <= S2_BOUND, (label, dS, dS2)
    return dS, dS2


def bitwise(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("n", "S", "S2", "rejected", "frame_obs"))


@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("name", ["rotating", "border", "clean640"])
def test_parity_with_the_statement(name, camera):
    import torch
    s = scene_of(name, camera)
    ref_plain, ref_clipped = statement(name, camera)
    frames = torch.from_numpy(s.frames).cuda()
    b = builder(s)
    parity(run_library(b, frames, s.poses), ref_plain, "%s / %s plain" % (name, camera))
    parity(run_library(b, frames, s.poses, clip=CLIP), ref_clipped, "%s / %s clipped" % (name, camera))
    b.close()


SHAPES = ["one_sample", "three_tags", "one_frame", "unused_frame", "nothing_visible", "pitch", "frame_stride"]


@pytest.mark.parametrize("shape", SHAPES)
def test_smallest_shapes(shape):
    import torch
    s = scene_of("rotating")
    F = len(s.poses)
    sel, frames_np, poses, use = None, s.frames, s.poses, None
    if shape == "one_sample":
        sel = np.array([137])
    elif shape == "three_tags":
        sel = np.flatnonzero(np.isin(s.tag, (0, 3, 7)))
        assert sel.size == 75
    elif shape == "one_frame":
        frames_np, poses = s.frames[4:5], s.poses[4:5]
    elif shape == "unused_frame":
        use = np.ones(F, np.uint8); use[[0, 5]] = 0
        poses = poses.copy(); poses[5] = np.nan                 # an unused pose is not looked at
    elif shape == "nothing_visible":
        # the body seen from behind in the call's only frame; then a call that does see it
        from scipy.spatial.transform import Rotation
        back = np.concatenate([(Rotation.from_euler("y", 180, degrees=True) * Rotation.from_rotvec(s.poses[4, :3])).as_rotvec(), s.poses[4, 3:]])
        frames_np, poses = s.frames[[4, 4]], np.stack([back, s.poses[4]])
    prob = s.problem(sel)
    ref_plain, ref_clipped = dm.learn(prob, frames_np, poses, use, *CLIP)
    assert dm.margins_ok(ref_clipped["margins"])
    h, w = s.height, s.width
    if shape == "pitch":
        buf = torch.full((len(frames_np), h, w + 13), 255, dtype=torch.uint8, device="cuda")           # poisoned padding
        buf[:, :, :w] = torch.from_numpy(frames_np).cuda()
        frames = buf[:, :, :w]
        assert frames.stride(1) == w + 13
    elif shape == "frame_stride":
        buf = torch.full((len(frames_np), h + 3, w + 13), 255, dtype=torch.uint8, device="cuda")
        buf[:, :h, :w] = torch.from_numpy(frames_np).cuda()
        frames = buf[:, :h, :w]
        assert frames.stride(0) != frames.stride(1) * h
    else:
        frames = torch.from_numpy(np.ascontiguousarray(frames_np)).cuda()
    b = builder(s, sel)
    cuts = [1] if shape == "nothing_visible" else None
    lib_plain = run_library(b, frames, poses, use, cuts)
    parity(lib_plain, ref_plain, shape + " plain")
    parity(run_library(b, frames, poses, use, cuts, CLIP), ref_clipped, shape + " clipped")
    if shape == "nothing_visible":
        assert lib_plain["frame_obs"][0] == 0 and lib_plain["frame_obs"][1] > 0
    if shape == "unused_frame":
        assert (lib_plain["frame_obs"][[0, 5]] == 0).all()
    b.close()


def test_chunking_invariance():
    """the same 9 frames as one call, as 4 + 5 and as nine calls; a second builder; a host array uploaded in chunks"""
    import torch
    s = scene_of("rotating")
    ref_plain, ref_clipped = statement("rotating")
    frames = torch.from_numpy(s.frames).cuda()
    got = []
    for cuts in (None, [4], list(range(1, 9))):
        b = builder(s)
        got.append((run_library(b, frames, s.poses, cuts=cuts), run_library(b, frames, s.poses, cuts=cuts, clip=CLIP)))
        b.close()
    b2 = builder(s)
    got.append((run_library(b2, s.frames, s.poses), run_library(b2, s.frames, s.poses, clip=CLIP)))        # numpy frames
    b2.close()
    for k, (plain, clipped) in enumerate(got):
        parity(plain, ref_plain, "chunking %d plain" % k)
        parity(clipped, ref_clipped, "chunking %d clipped" % k)
        assert bitwise(plain, got[0][0]) and bitwise(clipped, got[0][1]), "cut %d differs from the single call" % k


def test_clipped_pass_drops_the_occluder():
    import torch
    occ = scene_of("occluder")
    ref_plain, ref_clipped = statement("occluder")
    clean_plain, _ = statement("clean640")
    frames = torch.from_numpy(occ.frames).cuda()
    b = builder(occ)
    lib_plain = run_library(b, frames, occ.poses)
    lib_clipped = run_library(b, frames, occ.poses, clip=CLIP)
    b.close()
    parity(lib_plain, ref_plain, "occluder plain")
    parity(lib_clipped, ref_clipped, "occluder clipped")
    k = occ.tag == sc.OCCLUDED_TAG
    tc, tp, tf = dm.template(clean_plain)[k], dm.template(lib_plain)[k], dm.template(lib_clipped)[k]
    rms_plain, rms_clipped = np.sqrt(np.mean((tp - tc) ** 2)), np.sqrt(np.mean((tf - tc) ** 2))
    print("tag %d vs the clean template: plain %.3g, clipped %.3g gray levels RMS" % (sc.OCCLUDED_TAG, rms_plain, rms_clipped))
    assert rms_clipped <= 0.25 * rms_plain


def test_refusals():
    """one case per refusal of include/agt_model.h that a caller can cause: ERR_ARG (every listed cause), ERR_CAMERA, ERR_ORDER.  ERR_ALLOC
    and ERR_HIP report a failing HIP runtime; nothing within the library's limits makes an allocation fail, and no test breaks the
    runtime on purpose."""
    import ctypes
    import torch
    from accurate_aprilgroup_tracking_amd import modellib as ML
    s = scene_of("rotating")
    frames = torch.from_numpy(s.frames).cuda()

    def create(**kw):
        a = dict(cameraMatrix=s.K, distCoeffs=None, width=s.width, height=s.height, tag_corners=s.corners, model_xyz=s.xyz, sample_tag=s.tag,
                 max_view_deg=60.0, facing=1)
        a.update(kw)
        return ML.DenseModelHandle(**a)

    def code(fn):
        with pytest.raises(ML.ModelError) as e:
            fn()
        return e.value.code

    bad_tag = s.tag.copy(); bad_tag[7] = 12
    arg_cases = dict(sample_tag=bad_tag, max_view_deg=0.0, facing=0, width=16385, height=3, tag_corners=np.zeros((257, 4, 3), np.float32))
    for k, v in arg_cases.items():
        assert code(lambda: create(**{k: v})) == ML.ERR_ARG, k
    for v in (91.0, float("nan"), float("inf")):
        assert code(lambda: create(max_view_deg=v)) == ML.ERR_ARG
    assert code(lambda: create(distCoeffs=np.zeros(6))) == ML.ERR_CAMERA
    L = ML.lib()
    hp = ctypes.c_void_p()
    assert L.agt_dense_model_create(None, None, ctypes.byref(hp)) == ML.ERR_ARG and L.agt_dense_model_create(None, None, None) == ML.ERR_ARG

    h = create()
    ptr, pitch, fs = frames.data_ptr(), frames.stride(1), frames.stride(0)
    # order: nothing before begin_pass, no clipped pass without a reference
    assert code(lambda: h.accumulate(ptr, pitch, fs, 9, s.poses)) == ML.ERR_ORDER
    assert code(h.read) == ML.ERR_ORDER
    assert code(lambda: h.begin_pass(1.5, 4.0)) == ML.ERR_ORDER
    h.begin_pass()
    assert code(lambda: h.begin_pass(1.5, 4.0)) == ML.ERR_ORDER          # (a plain pass without an accumulate call is no reference)
    for cs, fl in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1.5, -1.0), (1.5, float("nan"))):
        assert code(lambda: h.begin_pass(cs, fl)) == ML.ERR_ARG
    assert code(lambda: h.accumulate(ptr, s.width - 1, fs, 9, s.poses)) == ML.ERR_ARG              # pitch < width
    assert code(lambda: h.accumulate(ptr, pitch, fs, 0, np.zeros((0, 6)))) == ML.ERR_ARG
    assert code(lambda: h.accumulate(ptr, pitch, fs, 4097, np.zeros((4097, 6)))) == ML.ERR_ARG
    assert code(lambda: h.accumulate(0, pitch, fs, 9, s.poses)) == ML.ERR_ARG                      # NULL frames
    assert L.agt_dense_model_accumulate(h.h, ctypes.c_void_p(ptr), pitch, fs, 9, None, None, None) == ML.ERR_ARG
    bad = s.poses.copy(); bad[3, 4] = np.inf
    assert code(lambda: h.accumulate(ptr, pitch, fs, 9, bad)) == ML.ERR_ARG                        # a used pose that is not finite
    use = np.ones(9, np.uint8); use[3] = 0
    # none of the refused calls left a trace: the pass equals the statement's with frame 3 unused
    obs = h.accumulate(ptr, pitch, fs, 9, bad, use)
    n, S, S2, rej = h.read()
    ref = dm.run_pass(s.problem(), s.frames, s.poses, use)
    parity(dict(n=n, S=S, S2=S2, rejected=rej, frame_obs=obs), ref, "after the refusals")
    h.begin_pass(1.5, 4.0)                                                                         # now there is a reference
    h.close()


def _corner_error(s, k, pose):
    return float(np.linalg.norm(pnp_numpy.project(s.obj, pose[:3], pose[3:], s.K, None) - synthetic.project(s.obj, s.rvecs[k], s.tvecs[k], s.K), axis=1).mean())


def test_learned_template_refines_a_held_out_frame():
    """learn from frames 1-8 of the seed-3 scene (60 degree gate, min_obs = 4, compaction), refine frame 0 photometrically alone"""
    import torch
    from accurate_aprilgroup_tracking_amd import cv_hip, dense_model
    seq = sc.sequence3()
    learn = sc.clean640()
    model = dense_model.build_dense_model(torch.from_numpy(learn.frames).cuda(), learn.poses, seq.group, seq.K, None, grid=8, max_view_deg=60.0,
                                          clip_sigma=1.5, sigma_floor=4.0, min_obs=4)
    _, ref = statement("clean640")
    assert np.array_equal(model.n, ref["n"]) and np.array_equal(model.usable, ref["n"] >= 4)
    assert np.abs(model.model_t[model.usable] - dm.template(ref)[model.usable].astype(np.float32)).max() <= 2e-5          # (f32 rounding of ~1e2)
    c = model.compact()
    print(model.report())
    assert c.model_xyz.shape[0] == int(model.usable.sum()) >= 500
    # the single-frame template the tests used so far: frame 1 sampled at its true pose, every sample
    uv = synthetic.project(learn.xyz.astype(np.float64), seq.rvecs[1], seq.tvecs[1], seq.K)
    single = np.nan_to_num(synthetic.sample_bilinear(seq.frame(1), uv), nan=128.0).astype(np.float32)
    ctx = cv_hip.Context(640, 480)
    frame0 = torch.from_numpy(seq.frame(0)[None]).cuda()
    truth = np.concatenate([seq.rvecs[0], seq.tvecs[0]])
    starts = sc.perturbed_starts(truth)
    errs = {}
    for label, xyz, t in (("learned", c.model_xyz, c.model_t), ("single frame", learn.xyz, single)):
        e0, e1 = [], []
        for p0 in starts:
            pose = torch.from_numpy(p0[None].copy()).cuda()
            ctx.dense_refine(frame0, torch.from_numpy(xyz).cuda(), torch.from_numpy(t).cuda(), pose, seq.K, None, iters=8, photo_weight=1.0)
            e0.append(_corner_error(seq, 0, p0)); e1.append(_corner_error(seq, 0, pose.cpu().numpy()[0]))
        errs[label] = (np.mean(e0), np.mean(e1))
        print("%s template: mean corner error %.4f px -> %.4f px (starts %s)" % (label, np.mean(e0), np.mean(e1), np.round(e0, 3)))
    ctx.close()
    assert errs["learned"][1] < 0.05


def test_through_the_tracker_and_the_tool(tmp_path):
    import torch
    import build_dense_model as tool
    from accurate_aprilgroup_tracking_amd import formats, hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    s = synthetic.Sequence(640, 480, n_tags=12, n_frames=10, seed=3)
    F = len(s)
    frames = torch.from_numpy(s.frames()).cuda()
    trk = StreamTracker(s.width, s.height, s.obj, s.K, None, n_streams=1)
    trk.pipeline(0)
    trk.reset(frames[0:1].contiguous(), torch.from_numpy(s.corners(0)[None]).cuda().contiguous())
    so = trk.new_state_buffer(F - 2)
    for k in range(1, F - 1):
        trk.step(frames[k:k + 1], so[k - 1])
    torch.cuda.synchronize()
    st = so.cpu().numpy()[:, 0]
    use = (st[:, H.ST_OK] != 0).astype(np.uint8)
    assert use.sum() >= 6
    # the recording: frames 1-8 with the tracker's own poses
    formats.save_april_group(tmp_path / "april_group.json", s.group)
    formats.save_camera_params(tmp_path / "CameraParams.npz", s.K, np.zeros(5))
    np.save(tmp_path / "frames.npy", s.frames()[1:F - 1])
    np.save(tmp_path / "poses.npy", st[:, :6])
    np.save(tmp_path / "use.npy", use)
    out = tmp_path / "dense_model.npz"
    assert tool.main(["--group", str(tmp_path / "april_group.json"), "--camera", str(tmp_path / "CameraParams.npz"), "--frames", str(tmp_path / "frames.npy"),
                      "--poses", str(tmp_path / "poses.npy"), "--use", str(tmp_path / "use.npy"), "--grid", "8", "--out", str(out)]) == 0
    model = formats.load_dense_model(out)
    assert model.model_xyz.shape == (768, 3) and model.settings["grid"] == 8 and model.frame_obs.shape == (F - 2,)
    compact = trk.load_dense_model(out, iters=4, photo_weight=0.05, reseed=True)
    assert compact.usable.all() and 500 <= compact.model_xyz.shape[0] == int(model.usable.sum())
    state = trk.new_state_buffer()
    dense = trk.step_dense(frames[F - 1:F], state)
    torch.cuda.synchronize()
    st9, dn = state.cpu().numpy()[0], dense.cpu().numpy()[0]
    assert np.isfinite(dn).all() and np.isfinite(st9).all() and st9[H.ST_OK] == 1.0 and dn[H.DN_REFINED] == 1.0
    # the record's valid count = the compacted samples inside the window by the statement (at the solved and at the refined pose: the
    # body is nowhere near the frame's edge)
    X = compact.model_xyz.astype(np.float64)
    for pose in (st9[:6], dn[:6]):
        uv = pnp_numpy.project(X, pose[:3], pose[3:], s.K, None)
        assert dense_numpy.window_margin(uv, s.width, s.height) > 1.0
        assert int(dn[H.DN_VALID]) == int(dense_numpy.valid_window(uv, s.width, s.height).sum())
    print("held-out frame %d: corner error of the solved pose %.4f px, of the refined pose %.4f px; photometric rms %.3f over %d samples" %
          (F - 1, _corner_error(s, F - 1, st9[:6]), _corner_error(s, F - 1, dn[:6]), dn[H.DN_PHOTO_RMS], int(dn[H.DN_VALID])))
