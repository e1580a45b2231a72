"""Scenes and the plain numpy statement of the tag-consensus rule (test_tag_consensus.py, test_gpu_tag_consensus.py): seeded, procedural.

A scene is one view of a `synthetic.make_april_group` body: exact projections + Gaussian corner noise, with some tags displaced AS WHOLE
TAGS (all four corners by one vector of 6 - 25 px) -- what a tag that slid onto a neighbour or an occluder looks like to the solve.
`rule()` is section 1 of the rule (include/agt_hip.h agt_solve_pnp_consensus) written out with two callables, a solver and a projector,
so that the same statement serves the CPU oracle and the device's own stateless calls.  `check_margins()` is the condition every scene
of these tests has to meet under the oracle alone: no residual near the threshold, no near-tie between the two best hypotheses.

The edge batches (EDGE_BATCHES, make_edge_batch) each reach one clause of the rule or one bound of the vote kernel (csrc/agt_project.hip
vote_stream) that the scenes above stay clear of:
  e_nonfinite    step 2: two candidate tags with a used image coordinate NaN / image point (inf, inf) are no hypotheses; their other
                 corners still vote
  e_noncoplanar  step 2, AGT_PNP_TOO_FEW: a tag of four non-coplanar corners is no hypothesis without a guess and one with it
  e_flag         step 2, AGT_PNP_SINGULAR: a finite hypothesis -- the guess itself, better than any tag's -- that only its flag disqualifies
  e_behind       step 3, Zc > 0: corners that project within tau of their image points from behind the camera
  e_tie          step 4: count and sum of squares tie exactly, the lower tag wins; the count sits on min_inliers (and one above: none)
  e_t64, _last   T = 64, n = 256: all four waves full, the last slot of every array; _last: the winner is tag 63
  e_t1           T = 1, n = 4
  e_cpt8         corners_per_tag = 8: non-planar units, the DLT start
  e_cpt80, 128   corners_per_tag > 64: the hypothesis launch on the four-wave kernel; 128: T = 2, one unit masked, 255 inliers
test_tag_consensus.py holds each of them to the oracle's table and shows, with rule(depth_clause=False) / rule(flag_clause=False), that
e_behind and e_flag would elect otherwise without their clause.
"""
import numpy as np

TAU = 2.0
MIN_INLIERS = 8
NOISE_PX = 0.05
SINGULAR, TOO_FEW = 1, 4


class Scene:
    def __init__(self, n_tags=12, seed=0, n_bad=0, width=640, height=480, dist="mild", noise=NOISE_PX, all_bad=False, z0=0.30,
                 group_seed=None, projector=None):
        """seed: pose, noise, which tags are displaced and where to; group_seed (default: seed): the body, so that the streams of a
        batch can share one object array.  projector(obj, rvec, tvec, K, dist) -> (n,2): exact projections for cameras the analytic
        five-coefficient projection does not cover."""
        from accurate_aprilgroup_tracking_amd import synthetic as syn
        self.group = syn.make_april_group(n_tags=n_tags, seed=seed if group_seed is None else group_seed)
        self.obj = syn.group_object_points(self.group).astype(np.float32)
        self.K = syn.camera_matrix(width, height)
        self.dist = syn.MILD_DIST if isinstance(dist, str) else dist
        rng = np.random.default_rng(1000 + seed)
        # the body faces the camera within a quarter of a radian: every tag of the 46-degree cap is seen at less than about 60 degrees
        self.rvec = rng.uniform(-0.25, 0.25, 3)
        self.tvec = np.array([0.01, -0.02, z0]) + rng.uniform(-0.01, 0.01, 3)
        if projector is not None:
            self.exact = np.asarray(projector(self.obj.astype(np.float64), self.rvec, self.tvec, self.K, self.dist), np.float64).reshape(-1, 2)
        else:
            assert np.size(self.dist) <= 5
            self.exact = syn.project(self.obj, self.rvec, self.tvec, self.K, self.dist)
        self.n_tags, self.n = n_tags, 4 * n_tags
        self.noise = rng.normal(0.0, noise, (self.n, 2))
        bad = np.arange(n_tags) if all_bad else np.sort(rng.choice(n_tags, n_bad, replace=False))
        self.bad_tags = bad
        # displacements: distinct points of a hexagonal lattice (pitch 5 px) in the annulus 6 .. 25 px -- any two displaced tags
        # disagree by 5 px or more, so no displaced tag's pose gathers votes from another's corners
        lat = np.array([(5.0 * (i + 0.5 * (j & 1)), 5.0 * 0.8660254037844386 * j) for i in range(-6, 7) for j in range(-6, 7)])
        r = np.hypot(lat[:, 0], lat[:, 1])
        lat = lat[(r >= 6.0) & (r <= 25.0)]
        self.shift = np.zeros((self.n, 2))
        for t, v in zip(bad, lat[rng.choice(lat.shape[0], len(bad), replace=False)]):
            self.shift[4 * t:4 * t + 4] = v
        self.clean = np.ones(self.n, bool)
        for t in bad:
            self.clean[4 * t:4 * t + 4] = False
        # the guess a tracker would hold: the truth, a little off
        self.guess = np.concatenate([self.rvec + 0.01, self.tvec + np.array([0.002, -0.002, 0.005])])

    def truth(self):
        return np.concatenate([self.rvec, self.tvec])

    def img(self):
        return (self.exact + self.noise + self.shift).astype(np.float32)


def rodrigues(r):
    r = np.asarray(r, np.float64).reshape(3)
    th = np.linalg.norm(r)
    if th < 1e-300:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.cos(th) * np.eye(3) + (1 - np.cos(th)) * np.outer(k, k) + np.sin(th) * Kx


def rule(obj, img, usable, solve_tag, project, cpt=4, tau=TAU, min_inliers=MIN_INLIERS, depth_clause=True, flag_clause=True):
    """Section 1 for one stream.  obj (n,3), img (n,2), usable (n,) bool.
    solve_tag(t) -> (pose (6,) f64, flags) of tag t's cpt points alone, or None when the solver produced nothing;
    project(pose) -> (n,2) f64 projections of all object points.
    -> dict(inliers (n,) bool, winner, count, n_cand, n_hyp, pose (winner's, or None), counts {t: count}, ssq {t: ssq}, d2 {t: (n,) f64}).
    depth_clause / flag_clause = False: the rule WITHOUT "Zc > 0" / without the flag test of step 2 -- what a kernel that forgot the clause
    would compute; the CPU tests show with them that an edge scene's outcome hangs on the clause."""
    n = obj.shape[0]
    T = n // cpt
    img64 = np.asarray(img, np.float64)
    obj64 = np.asarray(obj, np.float64)
    counts, ssqs, d2s, poses, inls = {}, {}, {}, {}, {}
    n_cand = 0
    for t in range(T):
        if not usable[t * cpt:(t + 1) * cpt].all():
            continue
        n_cand += 1
        res = solve_tag(t)
        if res is None:
            continue
        pose, flags = res
        if (flag_clause and (flags & (SINGULAR | TOO_FEW))) or not np.isfinite(pose).all():
            continue
        uv = np.asarray(project(pose), np.float64).reshape(n, 2)
        du, dv = uv[:, 0] - img64[:, 0], uv[:, 1] - img64[:, 1]
        d2 = du * du + dv * dv
        zc = obj64 @ rodrigues(pose[:3])[2] + pose[5]
        with np.errstate(invalid="ignore"):
            inl = usable & ((zc > 0.0) | (not depth_clause)) & (d2 < tau * tau)
        counts[t], ssqs[t], d2s[t], poses[t], inls[t] = int(inl.sum()), float(d2[inl].sum()), d2, pose, inl
    best = -1
    for t in sorted(counts):
        if best < 0 or counts[t] > counts[best] or (counts[t] == counts[best] and ssqs[t] < ssqs[best]):
            best = t
    if best >= 0 and counts[best] < min_inliers:
        best = -1
    return dict(inliers=inls[best] if best >= 0 else np.zeros(n, bool), winner=best, count=counts[best] if best >= 0 else 0,
                n_cand=n_cand, n_hyp=len(counts), pose=poses[best] if best >= 0 else None, counts=counts, ssq=ssqs, d2=d2s, sets=inls)


def check_margins(res, usable, tau=TAU, margin=0.05):
    """The scene condition: under every accepted hypothesis no usable corner's residual lies within `margin` px of tau, and the two best
    hypotheses do not tie on count with sums of squares closer than 1e-6 relative unless they elect the same set.
    -> the smallest distance of a residual from tau (px)."""
    closest = np.inf
    for t, d2 in res["d2"].items():
        d = np.sqrt(d2[usable & np.isfinite(d2)])
        if d.size:
            closest = min(closest, float(np.abs(d - tau).min()))
    assert closest > margin, "a residual lies %.4f px from the threshold" % closest
    order = sorted(res["counts"], key=lambda t: (-res["counts"][t], res["ssq"][t], t))
    if len(order) >= 2:
        a, b = order[0], order[1]
        if res["counts"][a] == res["counts"][b] and not np.array_equal(res["sets"][a], res["sets"][b]):
            rel = abs(res["ssq"][a] - res["ssq"][b]) / max(res["ssq"][a], res["ssq"][b], 1e-300)
            assert rel > 1e-6, "the two best hypotheses tie (count %d, ssq %g / %g)" % (res["counts"][a], res["ssq"][a], res["ssq"][b])
    return closest


def oracle_rule(oracle, obj, img, K, dist, usable=None, guess=None, cpt=4, tau=TAU, min_inliers=MIN_INLIERS, iters_out=None, flagged=None, **clauses):
    """rule() with the CPU oracle's solvePnP and projectPoints.  iters_out: dict that receives {t: LM iterations}.
    flagged: {t: (pose, flags) or None} -- what solve_tag reports for these tags instead of the oracle's solve (the oracle solves with an
    SVD and sets no flag: DESIGN.md, deviation 2)."""
    n = obj.shape[0]
    usable = np.ones(n, bool) if usable is None else usable

    def solve_tag(t):
        if flagged and t in flagged:
            return flagged[t]
        sl = slice(t * cpt, (t + 1) * cpt)
        try:
            if guess is not None:
                _, r, tv, it = oracle.solvePnP(obj[sl], img[sl], K, dist, guess[:3].copy().reshape(3, 1), guess[3:].copy().reshape(3, 1), True,
                                               return_iters=True)
            else:
                _, r, tv, it = oracle.solvePnP(obj[sl], img[sl], K, dist, return_iters=True)
        except ValueError:
            return None
        if iters_out is not None:
            iters_out[t] = it
        return np.concatenate([np.asarray(r, np.float64).ravel(), np.asarray(tv, np.float64).ravel()]), 0

    def project(pose):
        return oracle.projectPoints(np.asarray(obj, np.float64), pose[:3], pose[3:], K, dist)[0]

    return rule(obj, img, usable, solve_tag, project, cpt, tau, min_inliers, **clauses)


def oracle_refit(oracle, obj, img, K, dist, res):
    """step 6 with the oracle -> (pose (6,), LM iterations) or None without consensus"""
    if res["winner"] < 0:
        return None
    m = res["inliers"]
    p = res["pose"]
    _, r, tv, it = oracle.solvePnP(obj[m], img[m], K, dist, p[:3].copy().reshape(3, 1), p[3:].copy().reshape(3, 1), True, return_iters=True)
    return np.concatenate([np.asarray(r, np.float64).ravel(), np.asarray(tv, np.float64).ravel()]), it


# ---- the batches of the GPU tests (shared object array; per stream: image points, mask, guess).  The CPU test holds every one of them to
# check_margins under the oracle, with and without the guess.
# a small sensor tilt on top of mild lens terms: the 14-coefficient camera
TILT14 = np.array([[0.01, -0.005, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.004, -0.003]])
BATCHES = ("b3_n48", "b3_n48_masked", "b2_n240", "b1_n8", "b2_allbad", "b1_tilt")


class Batch:
    def __init__(self, scenes, mask=None, obj=None, img=None, expected=None, cpt=4, min_inliers=MIN_INLIERS, guess=None, flagged=None):
        """obj / img / expected / guess: arrays that replace what the scenes give (the edge batches edit them); cpt, min_inliers: the call's;
        flagged: {stream: {tag: (pose, flags)}} hypotheses the reference takes as given instead of solving them (e_flag)."""
        self.scenes = scenes
        self.obj = scenes[0].obj if obj is None else obj
        if obj is None:
            for s in scenes:
                assert np.array_equal(s.obj, self.obj)
        self.K, self.dist = scenes[0].K, scenes[0].dist
        self.B, self.n = len(scenes), self.obj.shape[0]
        self.img = np.stack([s.img() for s in scenes]) if img is None else img
        self.guess = np.stack([s.guess for s in scenes]) if guess is None else guess
        self.mask = mask            # [B, n] u8 or None
        self.cpt, self.min_inliers = cpt, min_inliers
        self.flagged = flagged or {}
        if expected is not None:
            self.expected = expected
        else:
            self.expected = np.stack([s.clean for s in scenes])
            if mask is not None:
                self.expected = self.expected & (mask != 0)
        assert self.img.shape == (self.B, self.n, 2) and self.expected.shape == (self.B, self.n) and self.n % cpt == 0

    def usable(self, b):
        return np.ones(self.n, bool) if self.mask is None else self.mask[b] != 0

    def obj_of(self, b):
        return self.obj

    def flagged_for(self, b, guess):
        """the hypotheses of stream b the reference takes as given: {tag: (pose, flags) | None}; a callable entry is given the guess flag"""
        f = self.flagged.get(b)
        return None if f is None else {t: (v(guess) if callable(v) else v) for t, v in f.items()}

    def reference(self, oracle, b, guess, iters_out=None, **clauses):
        """the oracle's rule for stream b (guess: bool) with the batch's cpt and min_inliers"""
        return oracle_rule(oracle, self.obj, self.img[b], self.K, self.dist, usable=self.usable(b), guess=self.guess[b] if guess else None,
                           cpt=self.cpt, min_inliers=self.min_inliers, iters_out=iters_out,
                           flagged=self.flagged_for(b, guess), **clauses)


class StackedBatch:
    """One-stream batches of one camera, size and call as the streams of ONE call in the [B][n][3] object form (obj_batch_stride = 3 n):
    obj is (B,n,3); a stream without a mask gets ones."""

    def __init__(self, parts):
        p0 = parts[0]
        for p in parts:
            assert p.B == 1 and p.n == p0.n and (p.cpt, p.min_inliers) == (p0.cpt, p0.min_inliers)
            assert np.array_equal(p.K, p0.K) and np.array_equal(p.dist, p0.dist)
        self.parts = parts
        self.B, self.n, self.cpt, self.min_inliers, self.K, self.dist = len(parts), p0.n, p0.cpt, p0.min_inliers, p0.K, p0.dist
        self.obj = np.stack([p.obj for p in parts])
        self.img = np.concatenate([p.img for p in parts])
        self.guess = np.concatenate([p.guess for p in parts])
        self.expected = np.concatenate([p.expected for p in parts])
        self.mask = np.concatenate([np.ones((1, p.n), np.uint8) if p.mask is None else p.mask for p in parts])

    def usable(self, b):
        return self.mask[b] != 0

    def obj_of(self, b):
        return self.obj[b]

    def reference(self, oracle, b, guess, iters_out=None, **clauses):
        return self.parts[b].reference(oracle, 0, guess, iters_out, **clauses)


def make_batch(kind, oracle=None):
    if kind in ("b3_n48", "b3_n48_masked"):
        sc = [Scene(12, seed=s, n_bad=nb, group_seed=0) for s, nb in ((0, 0), (1, 3), (2, 5))]
        mask = None
        if kind.endswith("masked"):
            # one corner of a clean tag of every stream is knocked out: the tag is no candidate, its other three corners still vote
            mask = np.ones((3, 48), np.uint8)
            for b, s in enumerate(sc):
                t = int(np.setdiff1d(np.arange(12), s.bad_tags)[1 + b])
                mask[b, 4 * t + (b + 1) % 4] = 0
        return Batch(sc, mask)
    if kind == "b2_n240":
        # 60 tags: 14,400 residuals per stream -- less corner noise and a longer view keep every one of them off the threshold
        return Batch([Scene(60, seed=s, n_bad=20, group_seed=0, noise=0.02, z0=0.40) for s in (5, 7)])
    if kind == "b1_n8":
        return Batch([Scene(2, seed=0, n_bad=0)])
    if kind == "b2_allbad":
        return Batch([Scene(12, seed=0, n_bad=0, group_seed=0), Scene(12, seed=1, all_bad=True, group_seed=0)])
    if kind == "b1_tilt":
        proj = lambda obj, r, t, K, d: oracle.projectPoints(obj, r, t, K, d)[0]
        return Batch([Scene(12, seed=1, n_bad=3, group_seed=0, dist=TILT14, projector=proj)])
    if kind in EDGE_BATCHES:
        return make_edge_batch(kind)
    raise KeyError(kind)


# ---- the edge batches: one clause of the rule, or one bound of the vote kernel's arrays, each (see the module docstring).  Every scene brings
# its own object array, expected inlier set and, where the call differs, cpt / min_inliers.
EDGE_BATCHES = ("e_nonfinite", "e_noncoplanar", "e_tie", "e_behind", "e_t64", "e_t64_last", "e_t1", "e_cpt8", "e_cpt80", "e_cpt128", "e_flag")
E_T64_WINNER = 25           # the oracle's winner of e_t64 (asserted on the CPU); e_t64_last swaps that tag into slot 63
E_FLAG_TAG = 6
E_FLAG_OFF = 1e-5           # e_flag's guess: the truth + this, per component (at 1e-4 the guess is a worse pose than the best tag's: 0.34 px rms)


def _clean_tags(sc):
    return np.setdiff1d(np.arange(sc.n_tags), sc.bad_tags)


def _one(sc, **kw):
    """a one-stream batch of an edited scene"""
    kw.setdefault("obj", sc.obj)
    kw.setdefault("img", sc.img())
    kw["img"] = kw["img"][None]
    if "expected" in kw:
        kw["expected"] = kw["expected"][None]
    if kw.get("mask") is not None:
        kw["mask"] = kw["mask"][None]
    return Batch([sc], **kw)


def make_edge_batch(kind):
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    if kind == "e_nonfinite":
        # step 2, "a pose number not finite": two candidate tags with one image coordinate NaN / one image point (inf, inf), both usable
        sc = Scene(12, seed=1, n_bad=3, group_seed=0)
        c = _clean_tags(sc)
        img, exp = sc.img(), sc.clean.copy()
        img[4 * c[2] + 1, 0] = np.nan
        img[4 * c[4] + 3] = np.inf
        exp[[4 * c[2] + 1, 4 * c[4] + 3]] = False
        return _one(sc, img=img, expected=exp)
    if kind == "e_noncoplanar":
        # step 2, AGT_PNP_TOO_FEW: four non-coplanar points have no start without a guess (the DLT wants six) and a solve with one
        sc = Scene(12, seed=1, n_bad=3, group_seed=0)
        t = int(_clean_tags(sc)[3])
        o64 = sc.obj.astype(np.float64)
        q = o64[4 * t:4 * t + 4]
        nrm = np.cross(q[1] - q[0], q[3] - q[0])
        o64[4 * t + 2] += 0.005 * nrm / np.linalg.norm(nrm)
        obj = o64.astype(np.float32)
        img = sc.img()
        img[4 * t + 2] = (syn.project(obj[4 * t + 2:4 * t + 3], sc.rvec, sc.tvec, sc.K, sc.dist)[0] + sc.noise[4 * t + 2]).astype(np.float32)
        return _one(sc, obj=obj, img=img, expected=sc.clean.copy())
    if kind == "e_tie":
        # step 4, "a remaining tie to the lower t": tags 5 and 9 are bit copies of tag 3's object points and undisplaced image points
        sc = Scene(12, seed=0, all_bad=True, group_seed=0)
        obj, img = sc.obj.copy(), sc.img()
        good = (sc.exact + sc.noise).astype(np.float32)[12:16]
        for t in (5, 9):
            obj[4 * t:4 * t + 4] = sc.obj[12:16]
            img[4 * t:4 * t + 4] = good
        exp = np.zeros(sc.n, bool)
        exp[20:24] = exp[36:40] = True
        return _one(sc, obj=obj, img=img, expected=exp)
    if kind == "e_behind":
        # step 3, "Zc > 0": the twin tags are the point reflections of two clean tags through the camera centre -- they project onto
        # the same image points from behind the camera.  One corner of each twin is masked: no candidate, three corners that vote
        sc = Scene(12, seed=2, n_bad=2, group_seed=0)
        c = _clean_tags(sc)
        R, t = rodrigues(sc.rvec), sc.tvec
        o64, img = sc.obj.astype(np.float64), sc.img()
        mask, exp = np.ones(sc.n, np.uint8), sc.clean.copy()
        for s, d in ((c[0], c[2]), (c[1], c[3])):
            pc = o64[4 * s:4 * s + 4] @ R.T + t
            o64[4 * d:4 * d + 4] = (-pc - t) @ R
            img[4 * d:4 * d + 4] = img[4 * s:4 * s + 4]
            mask[4 * d] = 0
            exp[4 * d:4 * d + 4] = False
        return _one(sc, obj=o64.astype(np.float32), img=img, mask=mask, expected=exp)
    if kind in ("e_t64", "e_t64_last"):
        # the bounds of the vote kernel's arrays: T = 64 (VOTE_TAGS), n = 256, four full waves; _last: the winner sits in slot 63
        sc = Scene(64, seed=7, n_bad=20, group_seed=0, noise=0.02, z0=0.40)
        obj, img, exp = sc.obj.copy(), sc.img(), sc.clean.copy()
        if kind == "e_t64_last":
            a, b = slice(4 * E_T64_WINNER, 4 * E_T64_WINNER + 4), slice(252, 256)
            for arr in (obj, img, exp):
                arr[a], arr[b] = arr[b].copy(), arr[a].copy()
        return _one(sc, obj=obj, img=img, expected=exp)
    if kind == "e_t1":
        return _one(Scene(1, seed=0), min_inliers=4)
    if kind == "e_cpt8":
        # corners_per_tag = 8: two tags make a unit, its eight points are not coplanar -- the DLT start instead of the homography's
        sc = Scene(12, seed=1, n_bad=0, group_seed=0)
        img, exp = sc.img(), np.ones(sc.n, bool)
        img[8:16] += np.float32(9.0)
        exp[8:16] = False
        return _one(sc, img=img, expected=exp, cpt=8, min_inliers=16)
    if kind == "e_cpt80":
        # corners_per_tag > 64: the hypothesis launch itself takes the four-wave kernel.  Two streams, one body
        scs = [Scene(60, seed=s, n_bad=0, group_seed=0, noise=0.02, z0=0.40) for s in (5, 7)]
        img = np.stack([s.img() for s in scs])
        img[:, 160:240, 1] += np.float32(6.0)
        exp = np.ones((2, 240), bool)
        exp[:, 160:240] = False
        return Batch(scs, img=img, expected=exp, cpt=80, min_inliers=80)
    if kind == "e_cpt128":
        sc = Scene(64, seed=5, n_bad=0, group_seed=0, noise=0.02, z0=0.40)
        mask, exp = np.ones(sc.n, np.uint8), np.ones(sc.n, bool)
        mask[200] = 0
        exp[200] = False
        return _one(sc, mask=mask, expected=exp, cpt=128, min_inliers=128)
    if kind == "e_flag":
        # step 2, AGT_PNP_SINGULAR on a FINITE pose: the four object corners of one tag are the origin, so the rotation columns of the
        # Jacobian are exact zeros, the first pivot of the damped system is 0 (1 + lambda), the step is zeroed and the hypothesis is the
        # guess itself -- here the truth + 1e-5, a better pose than any tag's: only the flag keeps it from winning.  Without a guess the
        # tag's planarity ratio is 0 / 0 and it has no start.  The oracle sets no flag: the reference is told what the tag reports
        sc = Scene(12, seed=1, n_bad=0, group_seed=0)
        t = E_FLAG_TAG
        obj, img, exp = sc.obj.copy(), sc.img(), np.ones(sc.n, bool)
        obj[4 * t:4 * t + 4] = 0.0
        img[4 * t:4 * t + 4] = np.float32([[40, 40], [80, 40], [80, 80], [40, 80]])
        exp[4 * t:4 * t + 4] = False
        rest = np.delete(np.arange(sc.n), np.arange(4 * t, 4 * t + 4))
        origin = syn.project(np.zeros((1, 3)), sc.rvec, sc.tvec, sc.K, sc.dist)
        others = np.concatenate([sc.exact[rest], origin])
        dmin = np.sqrt(((img[4 * t:4 * t + 4, None, :].astype(np.float64) - others[None]) ** 2).sum(axis=2)).min()
        assert dmin >= 30.0, "the zero tag's image points lie %.1f px from another point" % dmin
        guess = (sc.truth() + E_FLAG_OFF)[None]
        return _one(sc, obj=obj, img=img, expected=exp, guess=guess, flagged={0: {t: lambda g: (guess[0].copy(), SINGULAR) if g else None}})
    raise KeyError(kind)


# ---- the tracker's scene: a rendered 640 x 480 stream of the 12-tag body in which, from frame OCC_FROM on, fixed texture covers two tags.
# LK carries those tags' corners onto the texture, which does not move with the body: both tags slide as whole tags, track back fine
# (the texture is as trackable as a tag) and enter the solve with status 1.
OCC_FROM = 2
OCC_TAGS = (0, 7)
OCC_PAD = 14
TRACK_FRAMES = 4            # (from the fifth frame on a slid corner comes within 0.05 px of the threshold under some hypothesis: check_margins)
TRACK_SCENE = (640, 480, 0)         # width, height, seed
TRACK_SPEED = 1.25


class SlidingSequence:
    def __init__(self, width=TRACK_SCENE[0], height=TRACK_SCENE[1], seed=TRACK_SCENE[2], n_frames=TRACK_FRAMES, occluded=True,
                 speed=TRACK_SPEED, tags=OCC_TAGS):
        from accurate_aprilgroup_tracking_amd import synthetic as syn
        import fb_scenes
        self.seq = syn.Sequence(width, height, n_tags=12, n_frames=n_frames, seed=seed, speed=speed)
        self.width, self.height, self.occluded, self.tags = width, height, occluded, tags
        self.obj, self.K, self.dist, self.group = self.seq.obj, self.seq.K, self.seq.dist, self.seq.group
        self.rvecs, self.tvecs = self.seq.rvecs, self.seq.tvecs
        self._tex = fb_scenes.occluder_texture(width, height) if occluded else None
        self._frames = {}

    def __len__(self):
        return len(self.seq)

    def corners(self, k):
        return self.seq.corners(k)

    def frame(self, k):
        if k not in self._frames:
            f = self.seq.frame(k)
            if self.occluded and k >= OCC_FROM:
                f = f.copy()
                for t in self.tags:
                    c = self.seq.corners(k)[4 * t:4 * t + 4]
                    x0, y0 = np.maximum(np.floor(c.min(axis=0)).astype(int) - OCC_PAD, 0)
                    x1, y1 = np.ceil(c.max(axis=0)).astype(int) + OCC_PAD + 1
                    f[y0:y1, x0:x1] = self._tex[y0:y1, x0:x1]
            self._frames[k] = f
        return self._frames[k]

    def truth(self, k):
        return np.concatenate([self.rvecs[k].ravel(), self.tvecs[k].ravel()]).astype(np.float64)


def detector_class(tmp_path, sc, tag):
    """a PoseDetector subclass whose april_group.json is the scene's body"""
    import json
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    d = tmp_path / ("g_%s" % tag)
    d.mkdir(exist_ok=True)
    (d / "april_group.json").write_text(json.dumps(sc.group))

    class Det(PoseDetector):
        DIRPATH = str(d)
    return Det


def mirror_chain(oracle, sc, tmp_path, tag, consensus_px=None, k0=0, steps=None, fb_px=None, margins=True):
    """The stream's CPU chain from frame k0 on: oracle LK of the frame's whole live tags (sticky status; fb_px: the forward-backward
    composition of tests/fb_scenes.py) -> PoseDetector(backend="cv", cv=oracle)._estimate_pose, whose host rule does the consensus.
    With margins, every frame's vote is also held to check_margins (the same inputs through oracle_rule).
    -> list of dict(ntrack, too_few, ok, guided, err, pose, consensus, pts, status) per tracked frame."""
    import logging
    import fb_scenes
    from oracle import cv2_shim
    log = logging.getLogger("test"); log.setLevel(logging.CRITICAL)
    det = detector_class(tmp_path, sc, tag)(log, sc.K, sc.dist, True, cv=cv2_shim.make_cv2(), pnp_consensus_px=consensus_px)
    obj32 = sc.obj.astype(np.float32)
    n = obj32.shape[0]
    pts = sc.corners(k0).astype(np.float32).copy(); alive = np.ones(n, bool)
    pyr = oracle.Pyramid(sc.frame(k0), 21, 2)
    recs = []
    last = len(sc) - 1 if steps is None else k0 + steps
    for k in range(k0 + 1, last + 1):
        npyr = oracle.Pyramid(sc.frame(k), 21, 2)
        if fb_px:
            nx, status, _, _, _ = fb_scenes.oracle_fb(oracle, pyr, npyr, pts, fb_px, alive=alive)
        else:
            nx, status, _ = oracle.calcOpticalFlowPyrLK(pyr, npyr, pts, winSize=(21, 21), maxLevel=2)
            nx = nx.reshape(-1, 2); nx[~alive] = pts[~alive]
        nx = nx.astype(np.float32)
        alive = alive & status.ravel().astype(bool)
        whole = np.repeat(alive.reshape(-1, 4).all(axis=1), 4)
        il = [nx[4 * t:4 * t + 4].reshape(1, 4, 2) for t in range(n // 4) if whole[4 * t]]
        ol = [obj32[4 * t:4 * t + 4] for t in range(n // 4) if whole[4 * t]]
        guided = det.extrinsic_guess[0] is not None
        closest = None
        if consensus_px and margins and len(il) >= 2:
            g = None if not guided else np.concatenate([np.asarray(det.extrinsic_guess[0], np.float64).ravel(), np.asarray(det.extrinsic_guess[1], np.float64).ravel()])
            res = oracle_rule(oracle, obj32, nx, sc.K, sc.dist, usable=whole, guess=g, tau=consensus_px)
            closest = check_margins(res, whole, tau=consensus_px)
        det._estimate_pose(il if len(il) >= 2 else [], ol if len(il) >= 2 else [])
        solved = det.last_error is not None
        recs.append(dict(too_few=not solved, ok=bool(solved and det.last_error < 2), guided=bool(guided and solved), err=det.last_error,
                         pose=None if not solved else np.concatenate([det.last_pose[0].ravel(), det.last_pose[1].ravel()]).astype(np.float64),
                         consensus=det.last_consensus if consensus_px else None, pts=nx.copy(), status=alive.copy(), closest=closest))
        pts = nx; pyr = npyr
    return recs
