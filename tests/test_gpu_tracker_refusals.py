"""-m gpu: the return codes of the tracker's entry points, pinned call by call, and the launch form the options force.

test_refusals: every entry point of the tracker with each bad argument or state, in the order the library checks them, and the cases
where two things are wrong at once (the earlier check decides the code).  Every refused call is refused before anything is enqueued.
The expected codes were read from the entry points' checks as they stood before the tracker's host code was split into units, and
the test passed on that library first; the checks now live in csrc/agt_api_tracker.hip (the shared ones in frame_call_ok),
csrc/agt_api_live.hip (agt_track_host_frame) and csrc/agt_ctx.h (TrackOptions::fits_corners / dense_refusal).

test_option_forces_the_stage_by_stage_form: reproject, consensus and predict, each switched on alone under a pipeline depth >= 1, give
the records of depth 0 bit for bit (TrackOptions::stage_by_stage; the forward-backward check's case is
test_gpu_fb_check.py::test_tracker_with_the_check_matches_its_cpu_chain).

The shape is the smallest with the two-level pyramid: 128 x 96, max_level 2, window 21, two tags (8 corners) in a context of 16 points
and 2 streams."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, HT, N, MAX_POINTS, MAX_STREAMS, FRAMES = 128, 96, 8, 16, 2, 7
OK, ARG, ALLOC, DIST, NPOINTS, HIP, UNSUPPORTED, STATE = 0, -1, -2, -3, -4, -5, -6, -7
_D = object()          # "the valid argument"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def scenes():
    """two streams of one two-tag object, 7 frames of 128 x 96 (tags of ~14 px)"""
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    return [syn.Sequence(W, HT, n_tags=2, n_frames=FRAMES, seed=3 + b, group_seed=3, z0=0.15, supersample=2) for b in range(MAX_STREAMS)]


class Rig:
    """One context of the test's shape with valid arguments for every call; each method is the raw C call -> its return code."""
    _inputs = None

    def __init__(self, torch, scenes, win=21):
        from accurate_aprilgroup_tracking_amd import hiplib as H
        from accurate_aprilgroup_tracking_amd.cv_hip import Context
        self.ctx = Context(W, HT, max_level=2, win=win, max_points=MAX_POINTS, max_streams=MAX_STREAMS)
        self.L, self.h = self.ctx.L, self.ctx.h
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        s0 = scenes[0]
        if Rig._inputs is None:             # (read-only device inputs, uploaded once for every rig of the module)
            c0 = np.stack([sc.corners(0) for sc in scenes]).astype(np.float32)
            clip = np.stack([np.stack([sc.frame(k) for sc in scenes]) for k in range(FRAMES)])          # [7, 2, 96, 128]
            Rig._inputs = (dev(clip), {N: dev(c0), 6: dev(c0[:, :6])}, dev(s0.obj.astype(np.float32)),
                           dev(s0.obj[:4].astype(np.float32)), dev(np.full(4, 0.5, np.float32)), dev(np.ones((MAX_STREAMS, N), np.uint8)))
        self.clip, self.corners, self.obj, self.model_xyz, self.model_t, self.mask = Rig._inputs
        self.K = np.ascontiguousarray(s0.K, np.float64)
        self.so = torch.zeros((FRAMES, MAX_STREAMS, H.STATE_STRIDE), dtype=torch.float64, device="cuda")
        self.do = torch.zeros((FRAMES, MAX_STREAMS, H.DENSE_STRIDE), dtype=torch.float64, device="cuda")
        self.gray = torch.zeros((HT, W), dtype=torch.uint8, device="cuda")
        self.h_frame = np.ascontiguousarray(s0.frame(1)); self.h_state = np.zeros(H.STATE_STRIDE, np.float64)
        self.pitch, self.bstride, self.fstride = W, W * HT, W * HT * MAX_STREAMS
        torch.cuda.synchronize()

    def _h(self, h):
        return self.h if h is _D else h

    def frame(self, k=1, off=0):
        return C.c_void_p(self.clip[k].data_ptr() + off)

    @staticmethod
    def _p(t, default):
        t = default if t is _D else t
        return None if t is None else C.c_void_p(t.data_ptr())

    # ---- state
    def build(self, B=1):
        return self.L.agt_pyramid_build(self.h, 0, self.frame(0), self.pitch, self.bstride, B)

    def reset(self, h=_D, slot=0, corners=_D, obj=_D, n=N, B=1, K=_D, dist=None, ndist=0):
        K = self.K.ctypes.data_as(C.c_void_p) if K is _D else K
        return self.L.agt_tracker_reset(self._h(h), slot, self._p(corners, self.corners.get(n)), self._p(obj, self.obj), n, B, K, dist, ndist, 1)

    def tracked(self, B=1, n=N):
        rc = self.build(B)
        return rc if rc else self.reset(B=B, n=n)

    # ---- setters
    def options(self, h=_D, reproject=0, min_points=8, gate_px=2.0):
        return self.L.agt_tracker_options(self._h(h), reproject, min_points, gate_px)

    def tag_gate(self, cpt=4, h=_D):
        return self.L.agt_tracker_tag_gate(self._h(h), cpt)

    def fb_check(self, px=1.0, h=_D):
        return self.L.agt_tracker_fb_check(self._h(h), px)

    def visibility(self, cpt=4, deg=60.0, facing=1, h=_D):
        return self.L.agt_tracker_visibility(self._h(h), cpt, deg, facing)

    def consensus(self, cpt=4, px=2.0, min_inliers=4, h=_D):
        return self.L.agt_tracker_consensus(self._h(h), cpt, px, min_inliers)

    def predict(self, px=32.0, h=_D):
        return self.L.agt_tracker_predict(self._h(h), px)

    def pipeline(self, depth, h=_D):
        return self.L.agt_tracker_pipeline(self._h(h), depth)

    def dense(self, h=_D, xyz=_D, t=_D, M=4, iters=1, weight=0.05, reseed=1):
        return self.L.agt_tracker_dense(self._h(h), self._p(xyz, self.model_xyz), self._p(t, self.model_t), M, iters, weight, reseed)

    # ---- frames
    def track(self, h=_D, frame=_D, pitch=_D, bstride=_D, B=1, k=1):
        return self.L.agt_track_frame(self._h(h), self.frame(k) if frame is _D else frame, self.pitch if pitch is _D else pitch,
                                      self.bstride if bstride is _D else bstride, B, C.c_void_p(self.so[k - 1].data_ptr()))

    def track_many(self, h=_D, frame=_D, pitch=_D, fstride=_D, B=1, count=2):
        return self.L.agt_track_frames(self._h(h), self.frame(1) if frame is _D else frame, self.pitch if pitch is _D else pitch, self.bstride,
                                       self.fstride if fstride is _D else fstride, B, count, C.c_void_p(self.so.data_ptr()))

    def detected(self, h=_D, frame=_D, pitch=_D, B=1, corners=_D):
        return self.L.agt_track_frame_detected(self._h(h), self.frame(1) if frame is _D else frame, self.pitch if pitch is _D else pitch, self.bstride,
                                               B, self._p(corners, self.corners[N]), self._p(_D, self.mask), C.c_void_p(self.so.data_ptr()))

    def track_dense(self, h=_D, frame=_D, pitch=_D, B=1, do=_D):
        return self.L.agt_track_frame_dense(self._h(h), self.frame(1) if frame is _D else frame, self.pitch if pitch is _D else pitch, self.bstride,
                                            B, C.c_void_p(self.so.data_ptr()), self._p(do, self.do))

    def track_many_dense(self, h=_D, frame=_D, pitch=_D, fstride=_D, B=1, count=2, do=_D):
        return self.L.agt_track_frames_dense(self._h(h), self.frame(1) if frame is _D else frame, self.pitch if pitch is _D else pitch, self.bstride,
                                             self.fstride if fstride is _D else fstride, B, count, C.c_void_p(self.so.data_ptr()), self._p(do, self.do))

    def estimate(self, h=_D, img=_D, B=1):
        return self.L.agt_estimate_pose(self._h(h), self._p(img, self.corners[N]), self._p(_D, self.mask), B, C.c_void_p(self.so.data_ptr()))

    def host_frame(self, h=_D, h_frame=_D, channels=1, src_w=W, src_h=HT, undistort=0, roi_x=0, roi_y=0, gray=_D, h_state=_D):
        hf = C.c_void_p(self.h_frame.ctypes.data) if h_frame is _D else h_frame
        hs = C.c_void_p(self.h_state.ctypes.data) if h_state is _D else h_state
        return self.L.agt_track_host_frame(self._h(h), hf, channels, src_w, src_h, None, undistort, roi_x, roi_y, self._p(gray, self.gray), W, None, hs)

    # ---- state reads
    def rewind(self, h=_D):
        return self.L.agt_tracker_rewind(self._h(h))

    def state_read(self, h=_D, dst=_D, B=1):
        buf = C.create_string_buffer(MAX_STREAMS * self.L.agt_tracker_state_size())
        return self.L.agt_tracker_state_read(self._h(h), buf if dst is _D else dst, B)

    def buffers(self, h=_D):
        cp, sp = C.c_void_p(), C.c_void_p()
        return self.L.agt_tracker_buffers(self._h(h), C.byref(cp), C.byref(sp))


NAN, INF = float("nan"), float("inf")
OPTIONS_ON = {"fb_check": lambda r: r.fb_check(), "visibility": lambda r: r.visibility(), "consensus": lambda r: r.consensus(),
              "predict": lambda r: r.predict()}


def _table():
    """(name, [steps that must succeed], the call, its code).  A context is created per case."""
    T = []

    def case(name, prep, call, want):
        T.append((name, prep, call, want))

    pose_only = lambda r: r.reset(corners=None)               # estimate-only tracker: no frame, no corners
    pose_only6 = lambda r: r.reset(corners=None, n=6)
    trk1 = lambda r: r.tracked(1)
    trk2 = lambda r: r.tracked(2)
    model = lambda r: r.dense()

    # ---- agt_tracker_reset: handle / model / slot, corner count, whole tags per option, streams, pyramid of the slot, camera
    case("reset: null context", [], lambda r: r.reset(h=None), ARG)
    case("reset: null model", [], lambda r: r.reset(obj=None, corners=None), ARG)
    case("reset: slot 2", [], lambda r: r.reset(slot=2, corners=None), ARG)
    case("reset: slot -1", [], lambda r: r.reset(slot=-1, corners=None), ARG)
    case("reset: slot 2 and 3 corners", [], lambda r: r.reset(slot=2, n=3, corners=None), ARG)
    case("reset: 3 corners", [], lambda r: r.reset(n=3, corners=None), NPOINTS)
    case("reset: more corners than the context holds", [], lambda r: r.reset(n=MAX_POINTS + 1, corners=None), NPOINTS)
    case("reset: 3 corners and no stream", [], lambda r: r.reset(n=3, B=0, corners=None), NPOINTS)
    case("reset: 6 corners, no option", [], pose_only6, OK)
    case("reset: 6 corners under the tag gate", [lambda r: r.tag_gate()], pose_only6, NPOINTS)
    case("reset: 6 corners under the visibility rule", [lambda r: r.visibility()], pose_only6, ARG)
    case("reset: 6 corners under consensus", [lambda r: r.consensus()], pose_only6, ARG)
    case("reset: 6 corners under the tag gate and the visibility rule", [lambda r: r.tag_gate(), lambda r: r.visibility()], pose_only6, NPOINTS)
    case("reset: 6 corners under the tag gate and consensus", [lambda r: r.tag_gate(), lambda r: r.consensus()], pose_only6, NPOINTS)
    case("reset: 6 corners under the tag gate, no stream", [lambda r: r.tag_gate()], lambda r: r.reset(corners=None, n=6, B=0), NPOINTS)
    case("reset: 6 corners under the tag gate, slot without a pyramid", [lambda r: r.tag_gate()], lambda r: r.reset(n=6), NPOINTS)
    case("reset: no stream", [], lambda r: r.reset(B=0, corners=None), ARG)
    case("reset: more streams than the context holds", [], lambda r: r.reset(B=MAX_STREAMS + 1, corners=None), ARG)
    case("reset: too many streams, slot without a pyramid", [], lambda r: r.reset(B=MAX_STREAMS + 1), ARG)
    case("reset: corners, slot without a pyramid", [], lambda r: r.reset(), STATE)
    case("reset: corners, pyramid of fewer streams", [lambda r: r.build(1)], lambda r: r.reset(B=2), STATE)
    case("reset: corners, the other slot's pyramid", [lambda r: r.build(1)], lambda r: r.reset(slot=1), STATE)
    case("reset: slot without a pyramid and no camera matrix", [], lambda r: r.reset(K=None), STATE)
    case("reset: no camera matrix", [], lambda r: r.reset(K=None, corners=None), ARG)
    case("reset: 3 distortion coefficients", [], lambda r: r.reset(corners=None, ndist=3), DIST)
    case("reset: no camera matrix and 3 distortion coefficients", [], lambda r: r.reset(K=None, corners=None, ndist=3), ARG)
    case("reset: 4 distortion coefficients, null", [], lambda r: r.reset(corners=None, ndist=4), ARG)
    case("reset: with corners", [], trk2, OK)

    # ---- agt_tracker_options
    case("options: null context", [], lambda r: r.options(h=None), ARG)
    case("options: min_points 5", [], lambda r: r.options(min_points=5), ARG)
    case("options: min_points 257", [], lambda r: r.options(min_points=257), ARG)
    case("options: gate 0", [], lambda r: r.options(gate_px=0.0), ARG)
    case("options: gate NaN", [], lambda r: r.options(gate_px=NAN), ARG)
    case("options: valid", [trk1], lambda r: r.options(reproject=1, min_points=6, gate_px=1.5), OK)

    # ---- agt_tracker_tag_gate / _visibility / _consensus: arguments, then whole tags of a tracker that has its corner count
    case("tag_gate: null context", [], lambda r: r.tag_gate(h=None), ARG)
    case("tag_gate: 3 corners per tag", [], lambda r: r.tag_gate(3), ARG)
    case("tag_gate: 3 corners per tag, 6 corners", [pose_only6], lambda r: r.tag_gate(3), ARG)
    case("tag_gate: 6 corners", [pose_only6], lambda r: r.tag_gate(4), NPOINTS)
    case("tag_gate: off, 6 corners", [pose_only6], lambda r: r.tag_gate(0), OK)
    case("tag_gate: before any reset", [], lambda r: r.tag_gate(4), OK)
    case("tag_gate: 8 corners", [trk1], lambda r: r.tag_gate(4), OK)
    case("visibility: null context", [], lambda r: r.visibility(h=None), ARG)
    case("visibility: 3 corners per tag", [], lambda r: r.visibility(cpt=3), ARG)
    case("visibility: angle -1", [], lambda r: r.visibility(deg=-1.0), ARG)
    case("visibility: angle 91", [], lambda r: r.visibility(deg=91.0), ARG)
    case("visibility: angle NaN", [], lambda r: r.visibility(deg=NAN), ARG)
    case("visibility: facing 0", [], lambda r: r.visibility(facing=0), ARG)
    case("visibility: 6 corners", [pose_only6], lambda r: r.visibility(), ARG)
    case("visibility: off, 6 corners", [pose_only6], lambda r: r.visibility(deg=0.0), OK)
    case("visibility: 8 corners, 5 per tag", [trk1], lambda r: r.visibility(cpt=5), ARG)
    case("visibility: 8 corners", [trk1], lambda r: r.visibility(deg=90.0, facing=-1), OK)
    case("consensus: null context", [], lambda r: r.consensus(h=None), ARG)
    case("consensus: threshold -1", [], lambda r: r.consensus(px=-1.0), ARG)
    case("consensus: threshold NaN", [], lambda r: r.consensus(px=NAN), ARG)
    case("consensus: threshold infinite", [], lambda r: r.consensus(px=INF), ARG)
    case("consensus: 3 corners per tag", [], lambda r: r.consensus(cpt=3), ARG)
    case("consensus: 65 corners per tag", [], lambda r: r.consensus(cpt=65, min_inliers=65), ARG)
    case("consensus: fewer inliers than a tag has corners", [], lambda r: r.consensus(cpt=4, min_inliers=3), ARG)
    case("consensus: 6 corners", [pose_only6], lambda r: r.consensus(), ARG)
    case("consensus: off, 6 corners", [pose_only6], lambda r: r.consensus(px=0.0), OK)
    case("consensus: 8 corners", [trk1], lambda r: r.consensus(), OK)

    # ---- agt_tracker_fb_check / _predict / _pipeline / _dense
    case("fb_check: null context", [], lambda r: r.fb_check(h=None), ARG)
    case("fb_check: -1", [], lambda r: r.fb_check(-1.0), ARG)
    case("fb_check: NaN", [], lambda r: r.fb_check(NAN), ARG)
    case("fb_check: infinite", [], lambda r: r.fb_check(INF), ARG)
    case("fb_check: on, off", [trk1, lambda r: r.fb_check(1.0)], lambda r: r.fb_check(0.0), OK)
    case("predict: null context", [], lambda r: r.predict(h=None), ARG)
    case("predict: -1", [], lambda r: r.predict(-1.0), ARG)
    case("predict: NaN", [], lambda r: r.predict(NAN), ARG)
    case("predict: infinite", [], lambda r: r.predict(INF), ARG)
    case("predict: on, off", [trk1, lambda r: r.predict(32.0)], lambda r: r.predict(0.0), OK)
    case("pipeline: null context", [], lambda r: r.pipeline(1, h=None), ARG)
    case("pipeline: depth -1", [], lambda r: r.pipeline(-1), ARG)
    case("pipeline: depth 33", [], lambda r: r.pipeline(33), ARG)
    case("pipeline: depth 32", [], lambda r: r.pipeline(32), OK)
    case("pipeline: depth 0", [trk1], lambda r: r.pipeline(0), OK)
    case("pipeline: window 13, depth -1", "win13", lambda r: r.pipeline(-1), ARG)
    case("pipeline: window 13, depth 4", "win13", lambda r: r.pipeline(4), UNSUPPORTED)
    case("pipeline: window 13, depth 0", "win13", lambda r: r.pipeline(0), OK)
    case("dense: null context", [], lambda r: r.dense(h=None), ARG)
    case("dense: M -1", [], lambda r: r.dense(M=-1), ARG)
    case("dense: iters -1", [], lambda r: r.dense(iters=-1), ARG)
    case("dense: iters 1001", [], lambda r: r.dense(iters=1001), ARG)
    case("dense: weight -1", [], lambda r: r.dense(weight=-1.0), ARG)
    case("dense: weight NaN", [], lambda r: r.dense(weight=NAN), ARG)
    case("dense: samples without positions", [], lambda r: r.dense(xyz=None), ARG)
    case("dense: samples without intensities", [], lambda r: r.dense(t=None), ARG)
    case("dense: samples without iterations", [], lambda r: r.dense(iters=0), ARG)
    case("dense: off", [model], lambda r: r.dense(xyz=None, t=None, M=0, iters=0), OK)
    case("dense: on", [], model, OK)

    # ---- the frame entry points: handle and pointers, tracker state, streams, frame geometry
    for name, call, pointer in (("track", Rig.track, "frame"), ("detected", Rig.detected, "frame"), ("track_dense", Rig.track_dense, "frame"),
                                ("track_many_dense", Rig.track_many_dense, "frame")):
        prep = [trk1, model] if "dense" in name else [trk1]
        case(name + ": null context", [], lambda r, f=call: f(r, h=None), ARG)
        case(name + ": null frame", prep, lambda r, f=call: f(r, frame=None), ARG)
        case(name + ": null frame, no reset", [], lambda r, f=call: f(r, frame=None), ARG)
        case(name + ": no reset", [], lambda r, f=call: f(r), STATE)
        case(name + ": no reset, no stream", [], lambda r, f=call: f(r, B=0), STATE)
        case(name + ": no stream", prep, lambda r, f=call: f(r, B=0), ARG)
        case(name + ": two streams for a tracker of one", prep, lambda r, f=call: f(r, B=2), ARG)
        case(name + ": one stream for a tracker of two", [trk2] + prep[1:], lambda r, f=call: f(r, B=1), ARG)
        case(name + ": other streams and a pitch of 130 (one code for both)", prep, lambda r, f=call: f(r, B=2, pitch=130), ARG)
        case(name + ": pitch of 130", prep, lambda r, f=call: f(r, pitch=130), ARG)
        case(name + ": pitch below the width", prep, lambda r, f=call: f(r, pitch=W - 4), ARG)
        case(name + ": frame at an odd address", prep, lambda r, f=call: f(r, frame=r.frame(1, off=1)), ARG)
    case("track: batch stride of 2 mod 4", [trk1], lambda r: r.track(bstride=W * HT + 2), ARG)
    case("track: estimate-only tracker", [pose_only], lambda r: r.track(), STATE)
    case("track_dense: estimate-only tracker", [pose_only, model], lambda r: r.track_dense(), STATE)
    case("track_many_dense: estimate-only tracker", [pose_only, model], lambda r: r.track_many_dense(), STATE)
    case("detected: null corners", [trk1], lambda r: r.detected(corners=None), ARG)
    case("detected: null corners, no reset", [], lambda r: r.detected(corners=None), ARG)
    case("detected: estimate-only tracker of one stream, two streams", [pose_only], lambda r: r.detected(B=2), ARG)

    # agt_track_frames: its own arguments first (even without a context), then agt_track_frame's per frame
    case("track_many: count -1", [trk1], lambda r: r.track_many(count=-1), ARG)
    case("track_many: count -1, null context", [], lambda r: r.track_many(h=None, count=-1), ARG)
    case("track_many: frame stride of 2 mod 4", [trk1], lambda r: r.track_many(fstride=W * HT * 2 + 2), ARG)
    case("track_many: frame stride of 2 mod 4, no reset", [], lambda r: r.track_many(fstride=W * HT * 2 + 2), ARG)
    case("track_many: no frame, null context", [], lambda r: r.track_many(h=None, count=0), OK)
    case("track_many: no frame, no reset", [], lambda r: r.track_many(count=0), OK)
    case("track_many: null context", [], lambda r: r.track_many(h=None), ARG)
    case("track_many: null frames", [trk1], lambda r: r.track_many(frame=None), ARG)
    case("track_many: no reset", [], lambda r: r.track_many(), STATE)
    case("track_many: two streams for a tracker of one", [trk1], lambda r: r.track_many(B=2), ARG)
    case("track_many: pitch of 130", [trk1], lambda r: r.track_many(pitch=130), ARG)

    # the dense calls: pointers (and the clip's own arguments), the four options, state and model, streams, geometry
    for name, call in (("track_dense", Rig.track_dense), ("track_many_dense", Rig.track_many_dense)):
        case(name + ": null records", [trk1, model], lambda r, f=call: f(r, do=None), ARG)
        case(name + ": no model", [trk1], lambda r, f=call: f(r), STATE)
        case(name + ": no model, two streams for a tracker of one", [trk1], lambda r, f=call: f(r, B=2), STATE)
        case(name + ": no model, pitch of 130", [trk1], lambda r, f=call: f(r, pitch=130), STATE)
        for opt, on in OPTIONS_ON.items():
            case("%s: %s on" % (name, opt), [trk1, model, on], lambda r, f=call: f(r), UNSUPPORTED)
            case("%s: %s on, no model" % (name, opt), [trk1, on], lambda r, f=call: f(r), UNSUPPORTED)
            case("%s: %s on, no reset" % (name, opt), [on], lambda r, f=call: f(r), UNSUPPORTED)
            case("%s: %s on, two streams for a tracker of one" % (name, opt), [trk1, model, on], lambda r, f=call: f(r, B=2), UNSUPPORTED)
            case("%s: %s on, null records" % (name, opt), [trk1, model, on], lambda r, f=call: f(r, do=None), ARG)
    case("track_many_dense: count -1", [trk1, model], lambda r: r.track_many_dense(count=-1), ARG)
    case("track_many_dense: count -1, predict on", [trk1, model, OPTIONS_ON["predict"]], lambda r: r.track_many_dense(count=-1), ARG)
    case("track_many_dense: frame stride of 2 mod 4, no model", [trk1], lambda r: r.track_many_dense(fstride=W * HT * 2 + 2), ARG)
    case("track_many_dense: no frame, fb_check on", [trk1, model, OPTIONS_ON["fb_check"]], lambda r: r.track_many_dense(count=0), UNSUPPORTED)
    case("track_many_dense: no frame, no model", [trk1], lambda r: r.track_many_dense(count=0), STATE)
    case("track_many_dense: no frame", [trk1, model], lambda r: r.track_many_dense(count=0), OK)

    # ---- agt_estimate_pose
    case("estimate: null context", [], lambda r: r.estimate(h=None), ARG)
    case("estimate: null corners", [pose_only], lambda r: r.estimate(img=None), ARG)
    case("estimate: null corners, no reset", [], lambda r: r.estimate(img=None), ARG)
    case("estimate: no reset", [], lambda r: r.estimate(), STATE)
    case("estimate: no reset, no stream", [], lambda r: r.estimate(B=0), STATE)
    case("estimate: no stream", [pose_only], lambda r: r.estimate(B=0), ARG)
    case("estimate: more streams than the tracker has", [pose_only], lambda r: r.estimate(B=2), ARG)

    # ---- agt_tracker_rewind / _state_read / _buffers
    case("rewind: null context", [], lambda r: r.rewind(h=None), ARG)
    case("rewind: no reset", [], lambda r: r.rewind(), STATE)
    case("rewind: estimate-only tracker", [pose_only], lambda r: r.rewind(), STATE)
    case("rewind: no frame since the reset", [trk1], lambda r: r.rewind(), STATE)
    case("rewind: one frame", [trk1, lambda r: r.track()], lambda r: r.rewind(), OK)
    case("rewind: twice", [trk1, lambda r: r.track(), lambda r: r.rewind()], lambda r: r.rewind(), STATE)
    case("state_read: null context", [], lambda r: r.state_read(h=None), ARG)
    case("state_read: null destination", [pose_only], lambda r: r.state_read(dst=None), ARG)
    case("state_read: no reset", [], lambda r: r.state_read(), ARG)
    case("state_read: no stream", [pose_only], lambda r: r.state_read(B=0), ARG)
    case("state_read: more streams than the tracker has", [pose_only], lambda r: r.state_read(B=2), ARG)
    case("state_read: valid", [pose_only], lambda r: r.state_read(), OK)
    case("buffers: null context", [], lambda r: r.buffers(h=None), STATE)
    case("buffers: no reset", [], lambda r: r.buffers(), STATE)
    case("buffers: estimate-only tracker", [pose_only], lambda r: r.buffers(), OK)

    # ---- agt_track_host_frame: pointers and channel count, tracker of one stream, the gray form's geometry, the colour form's staging
    case("host_frame: null context", [], lambda r: r.host_frame(h=None), ARG)
    case("host_frame: null frame", [trk1], lambda r: r.host_frame(h_frame=None), ARG)
    case("host_frame: null gray buffer", [trk1], lambda r: r.host_frame(gray=None), ARG)
    case("host_frame: null record", [trk1], lambda r: r.host_frame(h_state=None), ARG)
    case("host_frame: two channels", [trk1], lambda r: r.host_frame(channels=2), ARG)
    case("host_frame: two channels, no reset", [], lambda r: r.host_frame(channels=2), ARG)
    case("host_frame: no reset", [], lambda r: r.host_frame(), STATE)
    case("host_frame: estimate-only tracker", [pose_only], lambda r: r.host_frame(), STATE)
    case("host_frame: tracker of two streams", [trk2], lambda r: r.host_frame(), STATE)
    case("host_frame: tracker of two streams, other frame size", [trk2], lambda r: r.host_frame(src_w=W + 4), STATE)
    case("host_frame: gray, other frame size", [trk1], lambda r: r.host_frame(src_w=W + 4), ARG)
    case("host_frame: gray, other frame height", [trk1], lambda r: r.host_frame(src_h=HT + 2), ARG)
    case("host_frame: gray with a region", [trk1], lambda r: r.host_frame(roi_x=4), ARG)
    case("host_frame: gray with undistortion", [trk1], lambda r: r.host_frame(undistort=1), ARG)
    case("host_frame: pageable colour frame without a staging buffer", [trk1], lambda r: r.host_frame(channels=3), ARG)
    return T


def test_refusals(torch_cuda, scenes):
    wrong = []
    table = _table()
    for name, prep, call, want in table:
        win13 = prep == "win13"
        r = Rig(torch_cuda, scenes, win=13 if win13 else 21)
        steps = [s(r) for s in ([] if win13 else prep)]
        got = call(r) if not any(steps) else None
        if any(steps) or got != want:
            wrong.append("%s: preparation %s, code %s, expected %d" % (name, steps, got, want))
        torch_cuda.cuda.synchronize()
        r.ctx.close()
    print("%d cases" % len(table))
    assert not wrong, "\n".join(wrong)


def _clip_records(torch, scenes, depth, option):
    """the records [6, 2, 16] of the two-stream clip through agt_track_frame at a pipeline depth, one option on"""
    r = Rig(torch, scenes)
    assert option(r) == OK and r.pipeline(depth) == OK and r.tracked(MAX_STREAMS) == OK
    for k in range(1, FRAMES):
        assert r.track(B=MAX_STREAMS, k=k) == OK
    assert r.L.agt_tracker_join(r.h) == OK
    torch.cuda.synchronize()
    rec = r.so[:FRAMES - 1].cpu().numpy().copy()
    r.ctx.close()
    return rec


@pytest.mark.parametrize("option", ["reproject", "consensus", "predict"])
def test_option_forces_the_stage_by_stage_form(torch_cuda, scenes, option):
    from accurate_aprilgroup_tracking_amd import hiplib as H
    on = {"reproject": lambda r: r.options(reproject=1), "consensus": OPTIONS_ON["consensus"], "predict": OPTIONS_ON["predict"]}[option]
    want = _clip_records(torch_cuda, scenes, 0, on)
    print(option, "depth 0: tracked", want[:, :, H.ST_NTRACK].astype(int).tolist(), "accepted", want[:, :, H.ST_OK].astype(int).tolist())
    assert (want[:, :, H.ST_NTRACK] > 0).all(), "every frame's record is written, with tracked corners"
    for depth in (1, 4):
        got = _clip_records(torch_cuda, scenes, depth, on)
        assert got.tobytes() == want.tobytes(), "%s, depth %d: records differ from depth 0's in %s" % (
            option, depth, np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:8].tolist())
