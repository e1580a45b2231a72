"""-m gpu: the frame-chained LK body (agt_lk_chain_body.h) against the serial form, bit for bit, at the sizes where the rotation
of its three accumulator slots can go wrong.

The iteration sums of a trip cross the four waves of a corner through three rotating LDS accumulators; the rotation never
restarts inside a launch, so it runs through level ends, frame ends, lost corners and re-staged tiles in whatever phase the
iteration counts leave it (the rule of the slots: comment at iter_sum2).  Here:

  frames   176 x 160 -- the smallest size whose level 2 (44 x 40) still holds one whole 44 B x 40 row tile, so the prefetch of the
           next frame's search tiles is live -- and 96 x 80, where level 2 holds no whole tile and every frame loads on demand;
           8 corners, 9 tracked frames, max_level 0, 1, 2
  depths   fused launches of 1, 2, 3 and 32 frames against the stage-by-stage mode (depth 0): records of every frame bit-identical,
           corners and status after the clip bit-identical to the CPU oracle's LK chain (all corners, lost ones included: a lost
           corner carries its position)
  clips    "plain": small motion.  "events": corner 7 sits on a flat patch (no usable level, lost in frame 1: the `continue` path
           from frame 2 on), the surroundings of corner 6 go flat in image 2 (lost in frame 3, `continue` path behind it), and two
           whole-frame steps of more than 9 px: with max_level 0 a window that moves more than the 9 px tile margin at level 0
           leaves the search box in the middle of the level (code 3: round the outer loop, tile re-staged)
  knobs    on the diagnostic library (child processes, as test_chain_give_up_is_fail_stop loads it): AGT_LK_EPS=0 with
           AGT_LK_MAX_COUNT = 1, 2, 3, 4 -- up to n trips per level; the trips per corner and frame, counted by the oracle, take
           every residue mod 3, and the rotation meets level entries, frame ends and launch ends in every phase
           (test_rotation_meets_every_phase asserts that from the counts)

The test pins behaviour, not a particular implementation of the exchange: it passes on any library whose results are those of
the oracle."""
import ctypes as C
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = 9                                       # tracked frames (the clip has NF + 1 images)
PAD, FLAT = 40, 15
SIZES = {(176, 160): 6, (96, 80): 2}         # (width, height) -> seed of the clip (chosen so that corner 6 is lost in frame 3: asserted below)
DEPTHS = (0, 1, 2, 3, 32)


def _texture(h, w, seed):
    """blocky random texture, smoothed: edges and corners at every scale the three pyramid levels see"""
    rng = np.random.default_rng(seed)
    t = np.zeros((h, w))
    for cell, amp in ((16, 90.0), (8, 60.0), (4, 40.0)):
        g = rng.uniform(-1, 1, (h // cell + 2, w // cell + 2))
        t += amp * np.kron(g, np.ones((cell, cell)))[:h, :w]
    for _ in range(2):                       # 3 x 3 box blur, twice
        p = np.pad(t, 1, mode="edge")
        t = sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0
    return t + 128.0


def _shifted(t, h, w, sx, sy):
    """the h x w view of texture t displaced by (sx, sy) px (bilinear)"""
    x0, y0 = int(np.floor(sx)), int(np.floor(sy))
    a, b = sx - x0, sy - y0
    crop = lambda dx, dy: t[PAD - y0 - dy:PAD - y0 - dy + h, PAD - x0 - dx:PAD - x0 - dx + w]
    return (1 - a) * (1 - b) * crop(0, 0) + a * (1 - b) * crop(1, 0) + (1 - a) * b * crop(0, 1) + a * b * crop(1, 1)


@functools.lru_cache(maxsize=None)
def make_clip(w, h, case):
    """-> images [NF + 1, h, w] u8, corners in image 0 [8, 2] f32: a textured plane that translates"""
    seed = SIZES[(w, h)]
    t = _texture(h + 2 * PAD, w + 2 * PAD, seed)
    steps = np.random.default_rng(seed + 1).uniform(-1.6, 1.6, (NF, 2))
    if case == "events":
        steps[4] = (10.5, -6.25)             # beyond the 9 px tile margin at level 0
        steps[6] = (-9.75, 5.5)
    pos = np.concatenate([np.zeros((1, 2)), np.cumsum(steps, 0)])
    # six corners in the left part of the frame, two on the right with room for their flat patches (window 21 + Scharr border: +-12 px)
    xs, ys = (0.22 * w, 0.38 * w, 0.54 * w), (0.30 * h, 0.68 * h)
    c0 = [(x, y) for y in ys for x in xs] + [(w - 20.0, 0.26 * h), (w - 20.0, 0.74 * h)]
    c0 = np.array([(x + 0.37 * i, y + 0.21 * i) for i, (x, y) in enumerate(c0)], np.float32)
    images = []
    for k in range(NF + 1):
        f = _shifted(t, h, w, pos[k, 0], pos[k, 1])
        if case == "events":
            cx, cy = c0[7] + pos[k]          # corner 7: flat in every image
            x0, y0 = int(cx) - FLAT, int(cy) - FLAT
            f[max(y0, 0):max(y0 + 2 * FLAT, 0), max(x0, 0):max(x0 + 2 * FLAT, 0)] = 97.0
            if k >= 2:                       # corner 6: from image 2 on the whole strip around and above it (wherever frame 2 leaves the corner, it is flat there)
                cx, cy = c0[6] + pos[k]
                f[:max(int(cy) + FLAT, 0), max(int(cx) - FLAT, 0):] = 97.0
        images.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return np.stack(images), c0


def oracle_chain(oracle, images, c0, max_level, criteria=(3, 30, 0.01)):
    """The tracker's LK chain on the CPU oracle (sticky status, a lost corner carries its position), one corner per call so that the
    oracle's development counters give the iterations of that corner: -> points [NF, n, 2] f32, alive [NF, n], trips [NF, n, levels].
    (The counter also counts an iteration that ends on a window wholly outside the image before it sums anything; the plain clip,
    whose counts are used, keeps every window inside: no corner is within 20 px of a border or moves more than 15 px.)"""
    L = oracle.lib()
    iters = (C.c_long * 8).in_dll(L, "cvo_dbg_iters")
    n = len(c0)
    pts, alive, pyr = c0.copy(), np.ones(n, bool), oracle.Pyramid(images[0])
    all_pts, all_alive, trips = [], [], np.zeros((len(images) - 1, n, max_level + 1), int)
    for k in range(1, len(images)):
        npyr = oracle.Pyramid(images[k])
        nx, st = pts.copy(), np.zeros(n, bool)
        for i in np.nonzero(alive)[0]:
            L.cvo_dbg_reset()
            x, s, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts[i:i + 1], maxLevel=max_level, criteria=criteria)
            st[i], nx[i] = bool(s.ravel()[0]), x.reshape(2)
            trips[k - 1, i] = [iters[l] for l in range(max_level + 1)]
        alive = alive & st
        pts, pyr = nx.astype(np.float32), npyr
        all_pts.append(pts.copy()); all_alive.append(alive.copy())
    return np.stack(all_pts), np.stack(all_alive), trips


def track(torch, images, c0, w, h, max_level):
    """the clip through StreamTracker at every depth -> {depth: (records [NF, 1, stride], corners [n, 2] f32, status [n] u8)}"""
    from accurate_aprilgroup_tracking_amd import hiplib as H
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    f = float(w)
    K = np.array([[f, 0, w / 2.0], [0, f, h / 2.0], [0, 0, 1.0]])
    obj = np.concatenate([(c0.astype(np.float64) - [w / 2.0, h / 2.0]) / f, np.zeros((len(c0), 1))], 1)       # the plane z = 0 seen from (0, 0, 1)
    frames = torch.from_numpy(images).cuda()
    out = {}
    for depth in DEPTHS:
        trk = StreamTracker(w, h, obj, K, None, n_streams=1, max_level=max_level)
        trk.pipeline(depth)
        trk.reset(frames[0:1].contiguous(), torch.from_numpy(c0[None]).cuda().contiguous())
        so = trk.new_state_buffer(NF)
        for k in range(1, NF + 1):
            trk.step(frames[k:k + 1], so[k - 1])
        trk.join()
        cp, sp = trk.corners()
        torch.cuda.synchronize()
        got_c = np.zeros((len(c0), 2), np.float32); got_s = np.zeros(len(c0), np.uint8)
        H.check(trk.ctx.L.agt_download(trk.ctx.h, got_c.ctypes.data_as(C.c_void_p), C.c_void_p(cp), got_c.nbytes), "agt_download")
        H.check(trk.ctx.L.agt_download(trk.ctx.h, got_s.ctypes.data_as(C.c_void_p), C.c_void_p(sp), got_s.nbytes), "agt_download")
        rec = so.cpu().numpy()
        assert not (rec[:, :, H.ST_FLAGS].astype(int) & H.TRK_CHAIN_TIMEOUT).any()
        out[depth] = (rec, got_c, got_s)
    return out


def check_against_oracle(out, pts, alive, what):
    """every depth: all corners and their status after the clip are the oracle's, the records of every frame those of depth 0"""
    for depth in DEPTHS:
        rec, got_c, got_s = out[depth]
        assert np.array_equal(got_s.astype(bool), alive[-1]), "%s depth %d: status" % (what, depth)
        assert np.array_equal(got_c.view(np.uint32), pts[-1].view(np.uint32)), "%s depth %d: corners" % (what, depth)
        assert np.array_equal(rec.view(np.uint64), out[0][0].view(np.uint64)), "%s depth %d: records" % (what, depth)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("max_level", [0, 1, 2])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_plain_clip(torch_cuda, oracle, size, max_level):
    w, h = size
    images, c0 = make_clip(w, h, "plain")
    pts, alive, trips = oracle_chain(oracle, images, c0, max_level)
    assert alive.all() and (trips.sum(-1) > 0).all()
    check_against_oracle(track(torch_cuda, images, c0, w, h, max_level), pts, alive, "plain %dx%d max_level %d" % (w, h, max_level))


@pytest.mark.parametrize("max_level", [0, 1, 2])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_lost_corners_flat_patch_and_big_motion(torch_cuda, oracle, size, max_level):
    w, h = size
    images, c0 = make_clip(w, h, "events")
    pts, alive, trips = oracle_chain(oracle, images, c0, max_level)
    # what the clip is meant to contain, from the oracle: corner 7's level 0 is not usable in frame 1 (with max_level 0: no iteration
    # at all) and it is carried from then on; corner 6 is tracked through frame 2 and lost in frame 3; the others live through both
    # big steps
    assert not alive[0, 7] and trips[0, 7, 0] == 0
    assert alive[1, 6] and not alive[2, 6], "corner 6 is lost in frame 3"
    assert alive[:, :6].all()
    flow = np.abs(np.diff(np.concatenate([c0[None], pts]), axis=0)).max(-1)              # [NF, n] px per frame
    print("%dx%d max_level %d: largest flow of a live corner %.2f px, trips per corner-frame %.1f" % (w, h, max_level, flow[alive].max(), trips.sum(-1)[alive].mean()))
    assert flow[alive].max() > 9.5, "a live corner moves beyond the 9 px tile margin in one frame"
    check_against_oracle(track(torch_cuda, images, c0, w, h, max_level), pts, alive, "events %dx%d max_level %d" % (w, h, max_level))


# ---- the diagnostic library with fixed iteration counts: one child process per count (a knob is read once per process)
_KNOB_CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.environ["AGT_REPO_ROOT"]); sys.path.insert(0, os.path.join(os.environ["AGT_REPO_ROOT"], "tests"))
from accurate_aprilgroup_tracking_amd import hiplib as H
H.LIB_PATH = os.path.join(os.environ["AGT_REPO_ROOT"], "accurate_aprilgroup_tracking_amd", "libagt_hip_dbg.so")
import torch
import test_gpu_lk_chain_slots as T
res = {}
for (w, h) in sorted(T.SIZES):
    images, c0 = T.make_clip(w, h, "plain")
    for ml in (0, 1, 2):
        for depth, (rec, c, s) in T.track(torch, images, c0, w, h, ml).items():
            res["rec_%d_%d_%d_%d" % (w, h, ml, depth)] = rec
            res["c_%d_%d_%d_%d" % (w, h, ml, depth)] = c
            res["s_%d_%d_%d_%d" % (w, h, ml, depth)] = s
np.savez(os.environ["AGT_TEST_OUT"], **res)
print("RESULT ok")
'''


@functools.lru_cache(maxsize=None)
def knob_run(n):
    dbg = os.path.join(ROOT, "accurate_aprilgroup_tracking_amd", "libagt_hip_dbg.so")
    if not os.path.exists(dbg):
        subprocess.check_call(["make", "-s", "-j", "8", "-C", os.path.join(ROOT, "accurate_aprilgroup_tracking_amd", "csrc"), "dbg"])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.npz")
        env = dict(os.environ, AGT_LK_EPS="0", AGT_LK_MAX_COUNT=str(n), AGT_REPO_ROOT=ROOT, AGT_TEST_OUT=path)
        res = subprocess.run([sys.executable, "-c", _KNOB_CHILD], env=env, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0 and "RESULT ok" in res.stdout, res.stderr[-2000:]
        with np.load(path) as z:
            return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def knob_oracle(w, h, max_level, n):
    from oracle import cvoracle
    cvoracle.build()
    images, c0 = make_clip(w, h, "plain")
    return oracle_chain(cvoracle, images, c0, max_level, criteria=(3, n, 0.0))


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_fixed_iteration_counts(torch_cuda, oracle, n):
    res = knob_run(n)
    for (w, h) in sorted(SIZES):
        for ml in (0, 1, 2):
            pts, alive, trips = knob_oracle(w, h, ml, n)
            assert alive.all() and trips.max() <= n and (trips == n).any()
            out = {d: (res["rec_%d_%d_%d_%d" % (w, h, ml, d)], res["c_%d_%d_%d_%d" % (w, h, ml, d)], res["s_%d_%d_%d_%d" % (w, h, ml, d)]) for d in DEPTHS}
            check_against_oracle(out, pts, alive, "max_count %d %dx%d max_level %d" % (n, w, h, ml))


def rotation_phases(trips, depth):
    """trips [NF, n, levels] of a clip tracked in launches of `depth` frames -> the phases (trips so far in the launch, mod 3) in which
    the corners' rotations meet a level's entry, the end of a frame inside a launch and the end of a launch, and the residues of
    the trips of one corner and frame"""
    level_entry, frame_end, launch_end, per_frame = set(), set(), set(), set()
    nf, n, nlev = trips.shape
    for i in range(n):
        for g0 in range(0, nf, depth):
            cum = 0
            for k in range(g0, min(g0 + depth, nf)):
                for l in range(nlev - 1, -1, -1):
                    if trips[k, i, l]:
                        level_entry.add(cum % 3)
                    cum += int(trips[k, i, l])
                per_frame.add(int(trips[k, i].sum()) % 3)
                (launch_end if k + 1 == min(g0 + depth, nf) else frame_end).add(cum % 3)
    return level_entry, frame_end, launch_end, per_frame


@pytest.mark.parametrize("max_level", [0, 1, 2])
@pytest.mark.parametrize("size", sorted(SIZES))
def test_rotation_meets_every_phase(oracle, size, max_level):
    """coverage of test_fixed_iteration_counts, from the oracle's iteration counts (every window of the plain clip stays inside its
    image -- no corner is lost --, so an iteration counted is a trip run): over the four counts and the fused depths, per size and
    max_level"""
    w, h = size
    sets = [set(), set(), set(), set()]
    for n in (1, 2, 3, 4):
        pts, alive, trips = knob_oracle(w, h, max_level, n)
        assert alive.all()
        for depth in DEPTHS[1:]:
            for s, got in zip(sets, rotation_phases(trips, depth)):
                s |= got
    print("%dx%d max_level %d: phases at level entries %s, frame ends %s, launch ends %s; trips per frame mod 3 %s" % ((w, h, max_level) + tuple(sorted(s) for s in sets)))
    assert all(s == {0, 1, 2} for s in sets)
