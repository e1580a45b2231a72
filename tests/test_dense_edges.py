"""Dense refinement (csrc/agt_dense.hip, agt_dense_body.h; entry agt_dense_refine) at the sizes the workload never reaches: the
sample tail, the second trips of the row loop and of the corner block, a frame pitch other than the width, samples at the frame
border and exactly on the validity boundary, the singular solve, the early stop and iters = 0.

Three implementations of the SPECIFICATION of oracle/cv_dense.c: tests/dense_numpy.py (float64 numpy, the reference of this file),
the C oracle and the HIP kernels.  The CPU half holds the oracle to the numpy statement on every scene and proves the scenes fit
for a comparison at 1e-9 (no sample within 1e-6 px of a validity boundary, cond(A) < 1e8, no stop-rule ratio within a factor 2
of FLT_EPSILON); the GPU half holds the kernels to both on the same scenes.  Tolerances are those of tests/test_dense.py: poses
1e-9, RMS 1e-8, counts equal (summation order costs ~1e-12).
"""
import numpy as np
import pytest

import dense_numpy
import pnp_numpy
from accurate_aprilgroup_tracking_amd import synthetic as syn

FLT_EPSILON = dense_numpy.FLT_EPSILON
W, H = 160, 120
K0 = np.array([[210.5, 0.0, 79.3], [0.0, 208.25, 60.7], [0.0, 0.0, 1.0]])
TRUE = np.array([0.10, -0.15, 0.05, 0.01, -0.02, 1.0])
TILT14 = np.array([[0.02, -0.01, 1e-3, -1e-3, 0.005, 0.01, -0.005, 0.002, 5e-4, -5e-4, 2e-4, 3e-4, 0.004, -0.003]])
POSE_TOL, RMS_TOL = 1e-9, 1e-8


# --------------------------------------------------------------------------- scene construction
def texture(seed, w=W, h=H, sigma=2.5):
    """Gaussian-smoothed random texture, stretched to the full u8 range"""
    from scipy.ndimage import gaussian_filter
    g = np.random.default_rng(seed).uniform(0.0, 1.0, (h, w))
    if sigma > 0:
        g = gaussian_filter(g, sigma, mode="wrap")
    return np.rint((g - g.min()) / (g.max() - g.min()) * 255.0).astype(np.uint8)


def plane_grid(M, half_x=0.22, half_y=0.16):
    """M samples of a regular grid on the plane z = 0 (evenly thinned when the grid has more nodes than M)"""
    if M == 0:
        return np.zeros((0, 3), np.float32)
    nx = int(np.ceil(np.sqrt(M * half_x / half_y)))
    ny = int(np.ceil(M / nx))
    idx = np.floor(np.arange(M) * (nx * ny / M)).astype(np.int64)
    ix, iy = idx % nx, idx // nx
    x = (ix + 0.5) / nx * 2 * half_x - half_x
    y = (iy + 0.5) / ny * 2 * half_y - half_y
    return np.stack([x, y, np.zeros(M)], 1).astype(np.float32)


def corner_set(N, K, dist, seed, B=1, noise=0.05):
    """N object points around the plane (some depth: the pose stays well determined by the corners alone) and their images at the
    true pose plus `noise` px, per stream"""
    rng = np.random.default_rng(seed)
    obj = np.stack([rng.uniform(-0.25, 0.25, N), rng.uniform(-0.18, 0.18, N), rng.uniform(-0.08, 0.08, N)], 1).astype(np.float32)
    uv = pnp_numpy.project(obj, TRUE[:3], TRUE[3:], K, dist)
    ipts = np.stack([uv + rng.normal(0, noise, uv.shape) for _ in range(B)]).astype(np.float32)
    return obj, ipts


def starts_near(B, seed, pose=TRUE):
    """B start poses less than 1 px off `pose` (asserted in the CPU half)"""
    rng = np.random.default_rng(seed)
    return np.stack([pose + rng.uniform(-1, 1, 6) * np.array([1.5e-3, 1.5e-3, 1.5e-3, 1e-3, 1e-3, 1e-3]) for _ in range(B)])


def template(frame, mx, K, dist, pose=TRUE):
    """template intensities: the frame sampled at the true pose (128 where the sample is invalid there)"""
    if len(mx) == 0:
        return np.zeros(0, np.float32)
    I, _, _, ok = dense_numpy.sample(frame, pnp_numpy.project(mx, pose[:3], pose[3:], K, dist))
    return np.where(ok, I, 128.0).astype(np.float32)


class Scene:
    """frames u8 [B, h, w]; mx f32 [M, 3], T f32 [M]; obj f32 [N, 3] / ipts f32 [B, N, 2] / mask u8 [B, N] or None; starts f64 [B, 6].
    kind: plain | border | exact | early | singular | noop.  pad: the device frames are a view of a larger tensor filled with 255."""

    def __init__(self, frames, mx, T, K, dist, starts, iters, pw, obj=None, ipts=None, mask=None, kind="plain", pad=False, expect=None):
        self.frames = np.ascontiguousarray(frames); self.mx = mx; self.T = T; self.K = K; self.dist = dist
        self.starts = np.ascontiguousarray(starts, dtype=np.float64); self.iters = iters; self.pw = pw
        self.obj = obj; self.ipts = ipts; self.mask = mask; self.kind = kind; self.pad = pad; self.expect = expect
        self.B = len(self.starts)
        assert self.frames.shape[0] == self.B and (ipts is None or ipts.shape[0] == self.B) and (mask is None or mask.shape[0] == self.B)

    def corners(self, b):
        if self.obj is None:
            return None, None, None
        return self.obj, self.ipts[b], None if self.mask is None else self.mask[b]


def _basic(M, N, B, iters, seed, dist=None, mask=None, pw=0.05, half=(0.22, 0.16), extra=None, **kw):
    """the common scene: one texture for every stream, the planar grid (+ `extra` samples), N corners, starts < 1 px off"""
    frame = texture(seed)
    mx = plane_grid(M, *half)
    if extra is not None:
        mx = np.concatenate([mx, extra.astype(np.float32)])
    obj, ipts = corner_set(N, K0, dist, seed + 1, B) if N else (None, None)
    return Scene(np.stack([frame] * B), mx, template(frame, mx, K0, dist), K0, dist, starts_near(B, seed + 2), iters, pw,
                 obj=obj, ipts=ipts, mask=mask, **kw)


def _corner_masks(N):
    """two streams: zeros on both sides of index 256 -- and at 255, 256 (where there is one) and N - 1"""
    rng = np.random.default_rng(N)
    m = (rng.uniform(size=(2, N)) > 0.25).astype(np.uint8)
    m[0, [3, 100, 255, N - 1]] = 0
    m[1, [0, 64, 254]] = 0; m[1, 255] = 1
    if N > 256:
        m[0, 256] = 0; m[1, 256] = 1
        if N > 258:
            m[1, [257, N - 2]] = 0; m[0, 258] = 1
        assert (m[0, 256:] == 0).any() and (m[1, 256:] != 0).any()
    assert (m[:, :256] == 0).any(axis=1).all() and not m[0, 255] and not m[0, N - 1]
    return m


def _border(dist, seed):
    # the plane overhangs all four frame edges (240 x 180 px of model on a 160 x 120 frame); 60 samples behind the camera, some
    # of which project INTO the frame: valid by the specification
    rng = np.random.default_rng(seed)
    behind = np.stack([rng.uniform(-0.3, 0.3, 60), rng.uniform(-0.2, 0.2, 60), rng.uniform(-3.0, -1.2, 60)], 1)
    return _basic(1500, 8, 1, 4, seed, dist=dist, half=(0.60, 0.45), extra=behind, kind="border")


def _exact(w, h, seed):
    # rvec = 0, tvec = (0, 0, 1), f = 64, integer principal point, model coordinates multiples of 1/64: u = 64 X + cx exactly, with
    # or without FMA.  16 samples on x0 in {0, 1, w - 3, w - 2} x y0 likewise (fewer distinct ones in the 4 x 4 frame)
    frame = texture(seed, w, h, sigma=0.0 if w < 16 else 2.5)
    cx, cy = w // 2, h // 2
    K = np.array([[64.0, 0.0, cx], [0.0, 64.0, cy], [0.0, 0.0, 1.0]])
    xs = sorted({0, 1, w - 3, w - 2}); ys = sorted({0, 1, h - 3, h - 2})
    uv = np.array([(x, y) for y in ys for x in xs], np.float64)
    mx = np.stack([(uv[:, 0] - cx) / 64.0, (uv[:, 1] - cy) / 64.0, np.zeros(len(uv))], 1).astype(np.float32)
    pose = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    assert np.array_equal(pnp_numpy.project(mx, pose[:3], pose[3:], K), uv)
    ok = dense_numpy.valid_window(uv, w, h)
    expect = int(((uv[:, 0] >= 1) & (uv[:, 0] <= w - 3) & (uv[:, 1] >= 1) & (uv[:, 1] <= h - 3)).sum())
    assert ok.sum() == expect == (1 if w == 4 else 4)
    T = (template(frame, mx, K, None, pose) + 3.0).astype(np.float32)
    rng = np.random.default_rng(seed)
    obj = np.stack([rng.uniform(-0.3, 0.3, 8), rng.uniform(-0.3, 0.3, 8), rng.uniform(-0.1, 0.1, 8)], 1).astype(np.float32)
    ipts = (pnp_numpy.project(obj, pose[:3], pose[3:], K) + rng.normal(0, 0.3, (8, 2))).astype(np.float32)[None]
    return Scene(frame[None], mx, T, K, None, pose[None], 1, 0.05, obj=obj, ipts=ipts, kind="exact", expect=expect)


def _all_invalid(iters):
    frame = texture(70)
    mx = plane_grid(300) + np.array([5.0, 0.0, 0.0], np.float32)             # ~1000 px to the right of the frame
    return Scene(np.stack([frame] * 2), mx, np.full(len(mx), 100.0, np.float32), K0, None, starts_near(2, 71), iters, 0.05, kind="singular")


def _converged(frame, mx, T, obj, ipts, mask, pw, pose):
    """the fixed point of the iteration: refine until the step is far below the stop rule's threshold"""
    for _ in range(6):
        r, t, _, d = dense_numpy.refine(frame, mx, T, obj, ipts, mask, K0, None, pose[:3], pose[3:], iters=60, photo_weight=pw)
        pose = np.concatenate([r, t])
    return pose


def _early_stop():
    # stream 0 starts at the optimum (stops after 1 iteration), stream 1 starts < 1 px off it and converges, stream 2 sees a
    # barely smoothed frame of another seed with every corner masked: its steps never fall under the threshold in 40
    smooth, rough = texture(80), texture(81, sigma=0.6)
    mx = plane_grid(1000)
    T = template(smooth, mx, K0, None)
    obj, ipts = corner_set(8, K0, None, 82, 3)
    mask = np.ones((3, 8), np.uint8); mask[2] = 0
    opt = _converged(smooth, mx, T, obj, ipts[0], None, 0.05, TRUE)
    ipts[1] = ipts[0]
    starts = np.stack([opt, starts_near(1, 87, opt)[0], starts_near(1, 85)[0]])
    return Scene(np.stack([smooth, smooth, rough]), mx, T, K0, None, starts, 40, 0.05, obj=obj, ipts=ipts, mask=mask, kind="early")


def _early_stop_corners_only():
    # the same without a single photometric block (M = 0): the geometric block is the only one, and the publishing one
    obj, ipts = corner_set(300, K0, None, 90, 2)
    opt = _converged(texture(91), np.zeros((0, 3), np.float32), np.zeros(0, np.float32), obj, ipts[0], None, 0.05, TRUE)
    return Scene(np.stack([texture(91)] * 2), np.zeros((0, 3), np.float32), np.zeros(0, np.float32), K0, None,
                 np.stack([opt, starts_near(1, 92)[0]]), 40, 0.05, obj=obj, ipts=ipts, kind="early")


def _pitch():
    # two different frames (the batch stride matters), the overhanging model (taps next to every frame edge)
    sc = _border(None, 40)
    f2 = texture(41)
    return Scene(np.stack([sc.frames[0], f2]), sc.mx, sc.T, K0, None, starts_near(2, 42), 4, 0.05, obj=sc.obj,
                 ipts=np.concatenate([sc.ipts, sc.ipts]), kind="border", pad=True)


SCENES = {}
for _M in (1, 63, 64, 65, 255, 256, 257, 1000):
    SCENES["tail-M%d" % _M] = (lambda M=_M: _basic(M, 8, 2, 3, 10 + M))
for _N in (0, 8):
    SCENES["rows-M65537-N%d" % _N] = (lambda N=_N: _basic(65537, N, 1, 3, 20 + N))
for _N in (256, 257, 300, 600):
    for _M in (1000, 0):
        SCENES["corners-N%d-M%d-masked" % (_N, _M)] = (lambda N=_N, M=_M: _basic(M, N, 2, 3, 30 + N, mask=_corner_masks(N)))
        SCENES["corners-N%d-M%d-nomask" % (_N, _M)] = (lambda N=_N, M=_M: _basic(M, N, 1, 3, 31 + N))
SCENES["pitch"] = _pitch
SCENES["border-pinhole"] = lambda: _border(None, 50)
SCENES["border-dist5"] = lambda: _border(syn.MILD_DIST, 51)
SCENES["border-tilt14"] = lambda: _border(TILT14, 52)
SCENES["exact-160x120"] = lambda: _exact(W, H, 60)
SCENES["exact-8x8"] = lambda: _exact(8, 8, 61)
SCENES["exact-4x4"] = lambda: _exact(4, 4, 62)
for _it in (1, 2, 5):
    SCENES["all-invalid-iters%d" % _it] = (lambda it=_it: _all_invalid(it))
SCENES["early-stop"] = _early_stop
SCENES["early-stop-corners-only"] = _early_stop_corners_only
SCENES["iters0"] = lambda: _basic(300, 8, 2, 0, 95, kind="noop")

_BUILT = {}


def _scene(name):
    """the scene and its numpy reference per stream, computed once and shared by every test (never modified)"""
    if name not in _BUILT:
        sc = SCENES[name]()
        ref = []
        for b in range(sc.B):
            o, ip, mk = sc.corners(b)
            ref.append(dense_numpy.refine(sc.frames[b], sc.mx, sc.T, o, ip, mk, sc.K, sc.dist, sc.starts[b, :3], sc.starts[b, 3:],
                                          iters=sc.iters, photo_weight=sc.pw))
        _BUILT[name] = (sc, ref)
    return _BUILT[name]


def _hold_to_reference(sc, ref, b, pose, stats, who):
    """pose (6,), stats (5+,) of one stream against the numpy statement: the bounds of the module docstring"""
    r, t, st, _ = ref[b]
    got = (int(stats[2]), int(stats[3]), int(stats[4]))
    want = (st["valid"], st["iters"], st["used"])
    d_pose = max(np.abs(pose[:3] - r).max(), np.abs(pose[3:] - t).max())
    d_rms = max(abs(stats[0] - st["photo_rms"]), abs(stats[1] - st["geo_rms"]))
    print("%s stream %d: (valid, iters, used) %s want %s, |pose - numpy| %.2e, |rms - numpy| %.2e" % (who, b, got, want, d_pose, d_rms))
    assert got == want, "%s stream %d: (valid, iters, used) %s, numpy %s" % (who, b, got, want)
    assert d_rms < RMS_TOL, "%s stream %d: rms off by %g" % (who, b, d_rms)
    assert d_pose < POSE_TOL, "%s stream %d: pose off by %g" % (who, b, d_pose)
    if sc.kind in ("singular", "noop"):
        assert np.array_equal(pose.view(np.uint64), sc.starts[b].view(np.uint64)), "%s stream %d: the pose must stay bit for bit" % (who, b)


# --------------------------------------------------------------------------- CPU half
@pytest.mark.parametrize("name", list(SCENES))
def test_oracle_equals_numpy_statement_and_scene_is_fit(oracle, name):
    """The C oracle against the numpy statement on every scene of this file -- and the conditions that make the scene fit for a
    comparison of two summation orders, asserted on the numpy statement alone."""
    sc, ref = _scene(name)
    M = len(sc.mx)
    for b in range(sc.B):
        r, t, st, dg = ref[b]
        # ---- the scene is fit
        if sc.kind != "exact":
            assert dg["margin"] > 1e-6, "a sample within %g px of a validity boundary" % dg["margin"]
        if sc.kind not in ("singular", "noop"):
            assert all(dg["solved"]) and max(dg["cond"]) < 1e8, "cond(A) = %g" % max(dg["cond"])
            # the stop rule cannot flip with the summation order: no ratio near the threshold before the last allowed iteration
            for k, q in enumerate(dg["ratio"]):
                assert k == sc.iters - 1 or q < 0.5 * FLT_EPSILON or q > 2 * FLT_EPSILON, "iteration %d: stop ratio %g" % (k, q)
            # starts are less than 1 px off the true pose (measured on what the true pose puts inside the frame, in front of the camera)
            if sc.kind != "exact":
                pts = np.concatenate([sc.mx.astype(np.float64), np.zeros((0, 3)) if sc.obj is None else sc.obj.astype(np.float64)])
                at_true = pnp_numpy.project(pts, TRUE[:3], TRUE[3:], sc.K, sc.dist)
                inside = (at_true[:, 0] > 0) & (at_true[:, 0] < W) & (at_true[:, 1] > 0) & (at_true[:, 1] < H)
                inside &= (pts @ pnp_numpy.rodrigues(TRUE[:3])[0].T + TRUE[3:])[:, 2] > 0
                d = pnp_numpy.project(pts[inside], sc.starts[b, :3], sc.starts[b, 3:], sc.K, sc.dist) - at_true[inside]
                assert inside.any() and np.abs(d).max() < 1.0
        if sc.kind == "border":
            assert 0.2 * M <= st["valid"] <= 0.8 * M, "%d of %d samples valid" % (st["valid"], M)
            Zc = (sc.mx.astype(np.float64) @ pnp_numpy.rodrigues(TRUE[:3])[0].T + TRUE[3:])[:, 2]
            uv = pnp_numpy.project(sc.mx, TRUE[:3], TRUE[3:], sc.K, sc.dist)
            front = uv[Zc > 0]
            assert (Zc <= 0).any() and dense_numpy.valid_window(uv[Zc <= 0], W, H).any()
            assert front[:, 0].min() < 0 and front[:, 0].max() > W and front[:, 1].min() < 0 and front[:, 1].max() > H
        if sc.kind == "exact":
            assert st["valid"] == sc.expect and st["iters"] == 1
        if sc.kind == "singular":
            assert dg["solved"] == [False] and (st["photo_rms"], st["geo_rms"], st["valid"], st["iters"], st["used"]) == (0, 0, 0, 1, 0)
            assert np.array_equal(np.concatenate([r, t]), sc.starts[b])
        if sc.kind == "noop":
            assert st == dict(photo_rms=0.0, geo_rms=0.0, valid=0, iters=0, used=0) and np.array_equal(np.concatenate([r, t]), sc.starts[b])
        if sc.kind == "early":
            q = dg["ratio"]
            if b == 0:
                assert st["iters"] == 1, "the stream that starts at the optimum stops at once"
            elif b == 1:
                assert 2 < st["iters"] < sc.iters, "the stream that starts off the optimum converges"
            else:
                assert st["iters"] == sc.iters and min(q) > 2 * FLT_EPSILON, "the third stream must not finish"
            if st["iters"] < sc.iters:
                assert q[-1] < 0.5 * FLT_EPSILON and (len(q) == 1 or q[-2] > 2 * FLT_EPSILON)
        # ---- the oracle follows the numpy statement
        o, ip, mk = sc.corners(b)
        ro, to, so = oracle.dense_refine(sc.frames[b], sc.mx, sc.T, o, ip, mk, sc.K, sc.dist, sc.starts[b, :3], sc.starts[b, 3:],
                                         iters=sc.iters, photo_weight=sc.pw)
        stats = np.array([so["photo_rms"], so["geo_rms"], so["valid"], so["iters"], so["used"]])
        _hold_to_reference(sc, ref, b, np.concatenate([ro, to]), stats, "oracle")


def test_the_scenes_reach_the_paths_they_are_built_for():
    """sizes only: what each group of scenes must exercise in agt_dense.hip / agt_dense_body.h"""
    for name in SCENES:
        if name.startswith("tail"):
            sc, _ = _scene(name)
            assert sc.B == 2 and not np.array_equal(sc.starts[0], sc.starts[1]) and len(sc.obj) == 8
    assert {len(_scene(n)[0].mx) for n in SCENES if n.startswith("tail")} == {1, 63, 64, 65, 255, 256, 257, 1000}
    for n in SCENES:
        if n.startswith("rows"):
            assert (len(_scene(n)[0].mx) + 255) // 256 == 257              # second trip of the update's row loop
        if n.startswith("corners") and n.endswith("masked"):
            sc, _ = _scene(n)
            assert sc.B == 2 and not np.array_equal(sc.mask[0], sc.mask[1]) and not sc.mask[0, 255] and not sc.mask[:, -1].all()
    sc, _ = _scene("pitch")
    assert sc.pad and not np.array_equal(sc.frames[0], sc.frames[1])


# --------------------------------------------------------------------------- GPU half
_CTX = []


def _hip(sc):
    """-> (pose [B, 6], stats [B, 8]) of Context.dense_refine on the scene, all streams in one call"""
    import torch
    from accurate_aprilgroup_tracking_amd import cv_hip
    if not _CTX:
        _CTX.append(cv_hip.Context(64, 64, max_level=0))
    frames = torch.from_numpy(sc.frames).cuda()
    if sc.pad:
        # a view of a larger tensor: pitch != w, a gap between the images, 255 wherever a stray tap could land
        B, h, w = sc.frames.shape
        big = torch.full((B, h + 7, w + 13), 255, dtype=torch.uint8, device="cuda")
        big[:, 3:3 + h, 5:5 + w] = frames
        frames = big[:, 3:3 + h, 5:5 + w]
        assert frames.stride(1) != w and frames.stride(0) != frames.stride(1) * h
    pose = torch.from_numpy(sc.starts.copy()).cuda()
    kw = {}
    if sc.obj is not None:
        kw = dict(obj=torch.from_numpy(sc.obj).cuda(), img_pts=torch.from_numpy(np.ascontiguousarray(sc.ipts)).cuda(),
                  mask=None if sc.mask is None else torch.from_numpy(np.ascontiguousarray(sc.mask)).cuda())
    pose, stats = _CTX[0].dense_refine(frames, torch.from_numpy(sc.mx).cuda(), torch.from_numpy(sc.T).cuda(), pose, sc.K, sc.dist,
                                       iters=sc.iters, photo_weight=sc.pw, **kw)
    return pose.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_hip_equals_numpy_statement(oracle, name):
    """The kernels against the numpy statement (and the oracle) on every scene: counts equal, poses to 1e-9, RMS to 1e-8; the pose
    bit for bit where nothing may move it (singular solve, iters = 0)."""
    sc, ref = _scene(name)
    pose, stats = _hip(sc)
    for b in range(sc.B):
        _hold_to_reference(sc, ref, b, pose[b], stats[b], "hip")
        assert (stats[b, 5:] == 0).all()
        o, ip, mk = sc.corners(b)
        ro, to, so = oracle.dense_refine(sc.frames[b], sc.mx, sc.T, o, ip, mk, sc.K, sc.dist, sc.starts[b, :3], sc.starts[b, 3:],
                                         iters=sc.iters, photo_weight=sc.pw)
        assert np.abs(pose[b] - np.concatenate([ro, to])).max() < POSE_TOL
        assert (int(stats[b, 2]), int(stats[b, 3]), int(stats[b, 4])) == (so["valid"], so["iters"], so["used"])
    if sc.kind == "noop":
        assert (stats == 0).all()
    if sc.kind == "singular":
        assert np.array_equal(stats[:, :5], np.tile([0.0, 0.0, 0.0, 1.0, 0.0], (sc.B, 1)))
    if sc.kind == "early":
        # launches after the stop return from the prologue: nothing moves, and a second call leaves the same bits
        pose2, stats2 = _hip(sc)
        assert np.array_equal(pose2.view(np.uint64), pose.view(np.uint64)) and np.array_equal(stats2.view(np.uint64), stats.view(np.uint64))
