"""StreamTracker: B independent streams tracked entirely on the device.

One `step(frames)` = pyramid(new frames) -> LK(previous corners) -> solvePnP(guess) ->
reprojection gate -> motion-model guess update, i.e. PoseDetector._estimate_pose
(detect_pose.py:467-574) fed by LK-tracked corners, with the PoseDetector state
(extrinsic_guess, prev_transform, velocity buffers) resident in HBM.  Four kernel launches
per step, no host<->device copy and no synchronisation; read `state` back when convenient.
"""
import ctypes as C
import numpy as np
import torch

from . import hiplib as H
from .cv_hip import Context, _ptr, _host_f64


class TrackState(C.Structure):
    """Mirror of csrc/agt_kernels.h AgtTrackState (tests read it back)."""
    _fields_ = [("guess", C.c_double * 6), ("prev", C.c_double * 6), ("rot_vel", (C.c_double * 9) * 2),
                ("tran_vel", (C.c_double * 3) * 2), ("prev_R", C.c_double * 9), ("has_guess", C.c_int), ("has_prev", C.c_int),
                ("n_vel", C.c_int), ("frame", C.c_int), ("guess_t_f32", C.c_int), ("prev_t_f32", C.c_int),
                ("chain_fault", C.c_int), ("pad", C.c_int)]


class _DeviceArray:
    """a library-owned device buffer as torch sees it (no copy, no ownership): the __cuda_array_interface__ of an address"""

    def __init__(self, address, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(address), False), "version": 2}


def _device_view(address, shape, typestr, device):
    return torch.as_tensor(_DeviceArray(address, shape, typestr), device=device)


class StreamTracker:
    def __init__(self, width, height, obj_points, K, dist=None, n_streams=1, max_level=2, win=21,
                 enhance_ape=True, reproject=False, min_points=8, gate_px=2.0, device=None, fb_check=0.0, view_deg=0.0, facing=1,
                 consensus_px=0.0, consensus_min=8, predict_px=0.0):
        if not (np.isfinite(predict_px) and predict_px >= 0):
            raise ValueError("StreamTracker: predict_px must be finite and >= 0")
        if view_deg and not reproject:
            # (the rule acts inside the reproject refresh only: accepting it here would be a silent no-op)
            raise ValueError("StreamTracker: view_deg needs reproject=True (the visibility rule acts in the corner refresh)")
        obj = np.ascontiguousarray(np.asarray(obj_points, np.float32).reshape(-1, 3))
        self.n = obj.shape[0]
        self.B = n_streams
        self.ctx = Context(width, height, max_level=max_level, win=win, max_points=max(self.n, 8),
                           max_streams=n_streams, device=device)
        self.dev = torch.device("cuda", self.ctx.device)
        self.obj = torch.from_numpy(obj).to(self.dev)
        self.K, _ = _host_f64(K)
        self.dist, self.ndist = _host_f64(dist)
        self.enhance_ape = bool(enhance_ape)
        self.reproject = bool(reproject)
        assert H.lib().agt_tracker_state_size() == C.sizeof(TrackState)
        H.check(self.ctx.L.agt_tracker_options(self.ctx.h, int(reproject), int(min_points), float(gate_px)),
                "agt_tracker_options")
        if fb_check:
            self.fb_check(fb_check)
        if view_deg:
            self.visibility(view_deg, 4, facing)
        if consensus_px:
            self.consensus(consensus_px, 4, consensus_min)
        if predict_px:
            self.predict(predict_px)
        self._alive = []            # frames aliased by pyramid level 0 of the ring entries in flight
        self._quad_detector = None  # detect_tags' workspace, made on first use
        self._keep_frames = max((max_level + 6) + 2, 12)

    def _dist_ptr(self):
        return self.dist.ctypes.data_as(C.c_void_p) if self.ndist else None

    def reset(self, frames=None, corners=None):
        """frames: cuda u8 [B,H,W] in which `corners` (cuda f32 [B,n,2]) were seen.  With both None
        only `estimate_pose` (detector-supplied corners) can be used afterwards."""
        self.ctx.use_current_stream()
        # (frames in flight come first -- slot 0 is a ring entry of the running tracker: agt_pyramid_build and
        # agt_tracker_reset both drain the pipeline themselves; reset is also the recovery from AGT_ERR_CHAIN)
        if frames is not None:
            self.ctx.pyramid_build(0, frames)
            assert corners.dtype == torch.float32 and corners.is_contiguous() and corners.shape == (self.B, self.n, 2)
        H.check(self.ctx.L.agt_tracker_reset(self.ctx.h, 0, _ptr(corners), _ptr(self.obj), self.n, self.B,
                                             self.K.ctypes.data_as(C.c_void_p), self._dist_ptr(), self.ndist,
                                             int(self.enhance_ape)), "agt_tracker_reset")
        self._alive = [frames]

    def pipeline(self, depth):
        """0 / False: separate launches per stage, pose complete in stream order.  F >= 1 (True = 1, the default):
        fused software-pipelined step advancing every stage by F frames per launch -- one launch every F calls
        of step(); the record of frame t is written about (L + 2) * F steps later (join() flushes)."""
        depth = int(depth)
        H.check(self.ctx.L.agt_tracker_pipeline(self.ctx.h, depth), "agt_tracker_pipeline")
        # (big batches run their stage kernels on library-owned streams: a frame is dead 9 calls after it was handed over)
        self._keep_frames = max((self.ctx.max_level + 6) * max(depth, 1) + 2, 12)

    def step(self, frames, state_out=None):
        """frames: cuda u8 [B,H,W] (a reference is kept while the frame is in flight: level 0 of the
        pyramid ring aliases it).  state_out: cuda f64 [B, STATE_STRIDE] or None; with the pipeline on
        it is written a few steps later -- call join() before consuming it.  Enqueues only."""
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.shape[0] == self.B
        assert tuple(frames.shape[1:]) == (self.ctx.height, self.ctx.width) and frames.stride(2) == 1, "frames must be [B, H, W] with unit pixel stride"
        H.check(self.ctx.L.agt_track_frame(self.ctx.h, _ptr(frames), frames.stride(1), frames.stride(0), self.B,
                                           _ptr(state_out)), "agt_track_frame")
        self._alive.append(frames)
        if len(self._alive) > self._keep_frames:
            del self._alive[0]
        return state_out

    def tag_gate(self, corners_per_tag=4):
        """4: the pose solve uses a corner only while all four corners of its tag are usable, min_points = 8 then is the
        reference's ">= 2 tags" (detect_pose.py:494-496).  0: every usable corner counts (the default of the C ABI)."""
        H.check(self.ctx.L.agt_tracker_tag_gate(self.ctx.h, int(corners_per_tag)), "agt_tracker_tag_gate")

    def fb_check(self, max_px=1.0):
        """Forward-backward check of the LK step: a corner whose track back from the new frame ends max_px (max norm) or more
        from where it started is treated as lost in that frame (status 0, sticky; out of the solve, the tag gate and NTRACK).
        0 switches it off (the default).  While it is on, step() runs stage by stage whatever the pipeline depth, with one
        more LK launch per frame; step_dense() is refused.  May be changed mid-stream; joins the pipeline."""
        H.check(self.ctx.L.agt_tracker_fb_check(self.ctx.h, float(max_px)), "agt_tracker_fb_check")

    def visibility(self, view_deg, corners_per_tag=4, facing=1):
        """Visibility rule of the reproject refresh (agt_tracker_visibility): on a closed body the refresh revives only the corners of
        tags whose centre is in front of the camera and whose outward normal (facing * (p3 - p0) x (p1 - p0)) is seen at less than
        view_deg (0, 90] from the viewing ray; the corners of the other tags get status 0 (their positions are still refreshed) and
        come back when the tag turns into view.  0 switches it off (the default).  Acts only with reproject=True; the record's
        ST_NVISIBLE slot counts the visible tags.  While it is on, step_dense() is refused.  May be changed mid-stream; joins the
        pipeline.  On a tracker built without reproject a non-zero view_deg raises ValueError, as in the constructor."""
        if view_deg and not self.reproject:
            raise ValueError("StreamTracker.visibility: view_deg needs reproject=True (the visibility rule acts in the corner refresh)")
        H.check(self.ctx.L.agt_tracker_visibility(self.ctx.h, int(corners_per_tag), float(view_deg), int(facing)), "agt_tracker_visibility")

    def consensus(self, inlier_px, corners_per_tag=4, min_inliers=8):
        """Tag consensus in front of the pose step (agt_tracker_consensus): every frame, each tag whose corners are all usable is solved
        alone (from the stream's guess when it has one), every usable corner votes on every tag's pose with the threshold inlier_px,
        and the pose step runs on status AND the winner's inliers -- a whole tag that slid consistently is outvoted by the others.  Per
        frame, not sticky: the status bytes are not rewritten; the record's ST_NINLIER slot carries the winning count, a frame whose
        best count is below min_inliers takes the too-few path.  inlier_px is not gate_px: the gate judges the mean error of the
        finished solve.  0 switches it off (the default).  While it is on, step() runs stage by stage whatever the pipeline depth,
        with two more launches per frame; step_dense() is refused.  May be changed mid-stream; joins the pipeline."""
        H.check(self.ctx.L.agt_tracker_consensus(self.ctx.h, int(corners_per_tag), float(inlier_px), int(min_inliers)), "agt_tracker_consensus")

    def predict(self, max_px=64.0):
        """Motion-predicted initial flow for the LK step (agt_tracker_predict): once a stream's last two records were both accepted, the
        constant-velocity extrapolation of their poses moves the start of every corner's search by the difference of its projections,
        so LK follows image motion far beyond its ~15 px reach.  A prediction with a corner behind the camera or a flow beyond max_px is
        distrusted as a whole and the frame is the plain step; the record's ST_FLOW slot carries the largest flow component (0.0 without
        a prediction, -1.0 when distrusted).  Assumes equal frame intervals; raw LK chaining still drifts under fast motion, so pair it
        with reproject=True on long stretches.  0 switches it off (the default).  While it is on, step() runs stage by stage whatever
        the pipeline depth, with one more launch per frame; step_dense() is refused.  May be changed mid-stream; joins the pipeline and
        clears the pose history."""
        if not (np.isfinite(max_px) and max_px >= 0):
            raise ValueError("StreamTracker.predict: max_px must be finite and >= 0")
        H.check(self.ctx.L.agt_tracker_predict(self.ctx.h, float(max_px)), "agt_tracker_predict")

    def rewind(self):
        """Take the newest frame back as the tracking source: the next step() tracks from the frame before it (the reference
        keeps the older frame as "previous" when a frame yields no tag, detect_pose.py:570-574).  Joins the pipeline."""
        H.check(self.ctx.L.agt_tracker_rewind(self.ctx.h), "agt_tracker_rewind")

    def step_detected(self, frames, corners, mask=None, state_out=None):
        """A detector-fed frame (detect_pose.py:576-609 with >= 2 tags found): `frames` joins the stream (the next step()
        tracks FROM it), `corners` cuda f32 [B,n,2] / `mask` cuda u8 [B,n] become its corner set and LK status and
        _estimate_pose runs on them.  Enqueues only; the record is complete in stream order."""
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.shape[0] == self.B
        assert tuple(frames.shape[1:]) == (self.ctx.height, self.ctx.width) and frames.stride(2) == 1, "frames must be [B, H, W] with unit pixel stride"
        assert corners.dtype == torch.float32 and corners.is_contiguous() and corners.shape == (self.B, self.n, 2)
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.shape == (self.B, self.n)
        H.check(self.ctx.L.agt_track_frame_detected(self.ctx.h, _ptr(frames), frames.stride(1), frames.stride(0), self.B,
                                                    _ptr(corners), _ptr(mask), _ptr(state_out)), "agt_track_frame_detected")
        self._alive.append(frames)
        if len(self._alive) > self._keep_frames:
            del self._alive[0]
        return state_out

    def step_many(self, clip, state_out=None):
        """A clip of consecutive frames in one call: clip cuda u8 [K,B,H,W], state_out cuda f64 [K,B,STATE_STRIDE] or None.
        Same as K calls of step() (same launches, same records) without the per-call host cost.  Enqueues only."""
        assert clip.dtype == torch.uint8 and clip.is_cuda and clip.dim() == 4 and clip.shape[1] == self.B
        assert tuple(clip.shape[2:]) == (self.ctx.height, self.ctx.width) and clip.stride(3) == 1, "clip frames must be H x W with unit pixel stride"
        K = clip.shape[0]
        if state_out is not None:
            assert state_out.is_contiguous() and tuple(state_out.shape) == (K, self.B, H.STATE_STRIDE)
        H.check(self.ctx.L.agt_track_frames(self.ctx.h, _ptr(clip), clip.stride(2), clip.stride(1), clip.stride(0), self.B, K,
                                            _ptr(state_out)), "agt_track_frames")
        self._alive.append(clip)                  # the whole clip stays referenced while any of its frames may be in flight
        while len(self._alive) > self._keep_frames:
            del self._alive[0]
        return state_out

    def dense_model(self, model_xyz, model_t, iters=5, photo_weight=0.05, reseed=True):
        """BASELINE configs[4]: register the dense model (cuda f32 [M,3] object-frame samples, cuda f32 [M] template
        intensities; kept alive here) -- step_dense() then refines every accepted pose photometrically on the device.
        model_xyz None disables the stage."""
        if model_xyz is None:
            H.check(self.ctx.L.agt_tracker_dense(self.ctx.h, None, None, 0, 0, 0.0, 0), "agt_tracker_dense")
            self._dense = None
            return
        assert model_xyz.dtype == torch.float32 and model_xyz.is_cuda and model_xyz.is_contiguous() and model_xyz.shape[1] == 3
        assert model_t.dtype == torch.float32 and model_t.is_cuda and model_t.is_contiguous() and model_t.shape[0] == model_xyz.shape[0]
        H.check(self.ctx.L.agt_tracker_dense(self.ctx.h, _ptr(model_xyz), _ptr(model_t), model_xyz.shape[0], int(iters),
                                             float(photo_weight), int(bool(reseed))), "agt_tracker_dense")
        self._dense = (model_xyz, model_t)

    def load_dense_model(self, model_or_path, iters=5, photo_weight=0.05, reseed=True):
        """Register a dense model learned from a recording (dense_model.build_dense_model, tools/build_dense_model.py): a
        dense_model.DenseModel or the .npz formats.save_dense_model wrote.  Its usable samples are uploaded and handed to
        dense_model().  -> the compacted DenseModel"""
        from . import dense_model as DM, formats
        model = model_or_path if isinstance(model_or_path, DM.DenseModel) else formats.load_dense_model(model_or_path)
        model = model.compact()
        if model.model_xyz.shape[0] == 0:
            raise ValueError("StreamTracker.load_dense_model: the model has no usable sample")
        self.dense_model(torch.from_numpy(model.model_xyz).to(self.dev), torch.from_numpy(model.model_t).to(self.dev), iters=iters,
                         photo_weight=photo_weight, reseed=reseed)
        return model

    def step_dense(self, frames, state_out=None, dense_out=None):
        """One frame with the dense stage: pyramid -> LK -> solvePnP(guess) + gate + motion model -> dense refinement of the
        accepted pose (-> corner re-seed).  dense_out: cuda f64 [B, DENSE_STRIDE] (created when None).  Enqueues only."""
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.shape[0] == self.B
        assert tuple(frames.shape[1:]) == (self.ctx.height, self.ctx.width) and frames.stride(2) == 1, "frames must be [B, H, W] with unit pixel stride"
        if dense_out is None:
            dense_out = torch.zeros((self.B, H.DENSE_STRIDE), dtype=torch.float64, device=self.dev)
        H.check(self.ctx.L.agt_track_frame_dense(self.ctx.h, _ptr(frames), frames.stride(1), frames.stride(0), self.B,
                                                 _ptr(state_out), _ptr(dense_out)), "agt_track_frame_dense")
        self._alive.append(frames)
        if len(self._alive) > self._keep_frames:
            del self._alive[0]
        return dense_out

    def step_many_dense(self, clip, state_out=None, dense_out=None):
        """A clip of consecutive frames with the dense stage in one call: clip cuda u8 [K,B,H,W], state_out cuda f64
        [K,B,STATE_STRIDE] or None, dense_out cuda f64 [K,B,DENSE_STRIDE] (created when None).  Same records as K calls of
        step_dense(); the library builds each next frame's pyramid inside the current frame's dense launch.  Enqueues only."""
        assert clip.dtype == torch.uint8 and clip.is_cuda and clip.dim() == 4 and clip.shape[1] == self.B
        assert tuple(clip.shape[2:]) == (self.ctx.height, self.ctx.width) and clip.stride(3) == 1, "clip frames must be H x W with unit pixel stride"
        K = clip.shape[0]
        if dense_out is None:
            dense_out = torch.zeros((K, self.B, H.DENSE_STRIDE), dtype=torch.float64, device=self.dev)
        assert dense_out.is_contiguous() and tuple(dense_out.shape) == (K, self.B, H.DENSE_STRIDE)
        if state_out is not None:
            assert state_out.is_contiguous() and tuple(state_out.shape) == (K, self.B, H.STATE_STRIDE)
        H.check(self.ctx.L.agt_track_frames_dense(self.ctx.h, _ptr(clip), clip.stride(2), clip.stride(1), clip.stride(0), self.B, K,
                                                  _ptr(state_out), _ptr(dense_out)), "agt_track_frames_dense")
        self._alive.append(clip)
        while len(self._alive) > self._keep_frames:
            del self._alive[0]
        return dense_out

    def join(self):
        """Enqueue the remaining pipeline stages of every supplied frame (no host synchronisation)."""
        H.check(self.ctx.L.agt_tracker_join(self.ctx.h), "agt_tracker_join")

    def estimate_pose(self, corners, mask=None, state_out=None):
        """PoseDetector._estimate_pose on device state with supplied corners (cuda f32 [B,n,2])."""
        assert corners.dtype == torch.float32 and corners.is_contiguous() and corners.shape == (self.B, self.n, 2)
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.shape == (self.B, self.n)
        H.check(self.ctx.L.agt_estimate_pose(self.ctx.h, _ptr(corners), _ptr(mask), self.B, _ptr(state_out)),
                "agt_estimate_pose")
        return state_out

    def estimate_pose_from_detections(self, detections_per_stream, tag_ids, state_out=None):
        """Detector-fed frame (detect_pose.py:389-437 -> :467-574): `detections_per_stream` holds, per stream,
        the swatbotics-style detections of this frame; `tag_ids` is the tag order of the object points.
        Builds the dense corner table + mask (formats.detections_to_corner_table) and runs the device
        state machine."""
        from . import formats
        tabs = [formats.detections_to_corner_table(d, tag_ids) for d in detections_per_stream]
        assert len(tabs) == self.B and tabs[0][0].shape[0] == self.n
        corners = torch.from_numpy(np.stack([t[0] for t in tabs])).to(self.dev)
        mask = torch.from_numpy(np.stack([t[1] for t in tabs])).to(self.dev)
        return self.estimate_pose(corners, mask, state_out)

    def decode_tags(self, frames, family, tag_ids=None, max_hamming=2, min_margin=0.0):
        """Image evidence that the tracked quads still show their tags (tag_decode, include/agt_tagcode.h): decodes the payload inside
        every tag of the tracker's own corner buffer in `frames` (cuda u8 [B,H,W], the frames the corners belong to -- the newest ones
        handed to step()), a tag being read only while all four of its corners have status 1.  family: a tag_decode.TagFamily; tag_ids:
        the family index of each tag of the model in model order (default 0..T-1).
        -> (records cuda u8 [B,T,40] -- tag_decode.records_numpy gives the fields --, corner_mask cuda u8 [B,n]): a tag's four mask
        bytes are 1 iff it decoded to its own id, unrotated, within max_hamming and at or above min_margin.  Feed the mask to
        step_detected(frames, corners, mask) or estimate_pose(corners, mask) to drop the tags that failed; step() is unchanged and
        never calls this.  Joins the pipeline; enqueues only."""
        from . import tag_decode
        assert self.n % 4 == 0, "decode_tags needs four corners per tag"
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.shape[0] == self.B
        assert tuple(frames.shape[1:]) == (self.ctx.height, self.ctx.width) and frames.stride(2) == 1, "frames must be [B, H, W] with unit pixel stride"
        T = self.n // 4
        ids = np.arange(T, dtype=np.int32) if tag_ids is None else np.ascontiguousarray(np.asarray(tag_ids, np.int32).reshape(-1))
        assert ids.size == T, "one family index per tag of the model"
        self.join()
        cp, sp = self.corners()
        quads = _device_view(cp, (self.B, T, 4, 2), "<f4", self.dev)
        mask = _device_view(sp, (self.B, T, 4), "|u1", self.dev).amin(dim=2)
        out = tag_decode.decode_quads(frames, quads, family, mask=mask, expected=torch.from_numpy(ids).to(self.dev),
                                      max_hamming=max_hamming, min_margin=min_margin)
        return out.records, out.corner_mask

    def refine_tags(self, frames, range_px=2.0, iters=2, min_strength=40.0):
        """The tracked quads snapped back onto the image (quad_refine, include/agt_quadfit.h): fits every tag of the tracker's own
        corner buffer to its border edges in `frames` (cuda u8 [B,H,W], the frames the corners belong to -- the newest ones handed to
        step()), a tag being fitted only while all four of its corners have status 1.
        -> (records cuda u8 [B,T,32] -- quad_refine.records_numpy gives the fields --, corners cuda f32 [B,n,2], corner_mask cuda u8
        [B,n]): a tag's four mask bytes are 1 iff it was refined; the corners of any other tag are the buffer's own.  The result is
        meant for step_detected(frames, corners, corner_mask) or estimate_pose(corners, corner_mask); tag_decode.decode_quads on
        corners.view(B, T, 4, 2) may come first, its mask ANDed with this one.  step() is unchanged and never calls this.  Joins the
        pipeline; enqueues only."""
        from . import quad_refine
        assert self.n % 4 == 0, "refine_tags needs four corners per tag"
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.shape[0] == self.B
        assert tuple(frames.shape[1:]) == (self.ctx.height, self.ctx.width) and frames.stride(2) == 1, "frames must be [B, H, W] with unit pixel stride"
        T = self.n // 4
        self.join()
        cp, sp = self.corners()
        quads = _device_view(cp, (self.B, T, 4, 2), "<f4", self.dev)
        mask = _device_view(sp, (self.B, T, 4), "|u1", self.dev).amin(dim=2)
        out = quad_refine.refine_quads(frames, quads, mask=mask, range_px=range_px, iters=iters, min_strength=min_strength)
        return out.records, out.quads.view(self.B, self.n, 2), out.corner_mask

    def detect_tags(self, frames, family, tag_ids=None, max_hamming=2, min_margin=0.0):
        """The model's tags found in `frames` (cuda u8 [B,H,W]) with no corner to start from (tag_detect: find -> refine -> decode,
        include/agt_quadfind.h, agt_quadfit.h, agt_tagcode.h): how a tracker that has no body yet, or lost it, (re-)acquires on the
        device.  family: a tag_decode.TagFamily; tag_ids: the family index of each tag of the model in model order (default 0..T-1).
        -> (corners cuda f32 [B,n,2], corner_mask cuda u8 [B,n], records cuda u8 [B,Q,40] -- tag_decode.records_numpy gives the fields,
        one per candidate slot of the finder): every candidate that decoded to a tag of the model is written into that tag's rows,
        its corners rolled by the decoded rotation into model order; of two candidates with one id the larger margin wins, on a tie
        the lower candidate index; every other tag's mask bytes are 0.  The result is what step_detected(frames, corners,
        corner_mask) takes.  The tracker's own corner buffer is neither read nor written; step() is unchanged and never calls this.
        Enqueues only."""
        from . import quad_detect, tag_detect
        assert self.n % 4 == 0, "detect_tags needs four corners per tag"
        assert frames.dtype == torch.uint8 and frames.is_cuda and frames.shape[0] == self.B
        assert tuple(frames.shape[1:]) == (self.ctx.height, self.ctx.width) and frames.stride(2) == 1, "frames must be [B, H, W] with unit pixel stride"
        T = self.n // 4
        lut = tag_detect.family_lut(family, tag_ids, T, self.dev)
        if self._quad_detector is None:
            self._quad_detector = quad_detect.QuadDetector(self.ctx.width, self.ctx.height, max_batch=self.B)
        tags = tag_detect.detect_tags(frames, family, detector=self._quad_detector, max_hamming=max_hamming, min_margin=min_margin)
        corners, mask = tag_detect.corner_table(tags, lut, T)
        return corners, mask, tags.decoded.records

    def draw_overlay(self, frames_bgr, draw_frames, state, radius=5, thickness=5, obj=None):
        """The reference's two images of a frame (detect_pose.py:441-465; overlay.draw_pose, include/agt_draw.h) without the pose leaving
        the device: the model is projected at the poses of `state` -- a record block cuda f64 [B, STATE_STRIDE] that step() (or
        step_detected / estimate_pose) filled; with the pipeline on, join() first --, a dot is painted on every projected corner into
        frames_bgr (cuda u8 [B,H,W,3] or [B,H,W], in place) and the tag outlines on draw_frames (same layout), which are cleared first.
        A stream whose record is not accepted (ST_OK is not 1) keeps its frame untouched and gets a black drawing frame.  obj: the model
        points to project, cuda f32 or f64 [n,3] (default: the tracker's own f32 copy).  -> the projected points cuda [B,n,2].
        Enqueues on the tracker's stream; nothing is read back and nothing synchronises.  step() never calls this."""
        from . import overlay
        assert state.is_cuda and state.dtype == torch.float64 and tuple(state.shape) == (self.B, H.STATE_STRIDE) and state.stride(1) == 1
        assert self.n % 4 == 0, "draw_overlay needs four corners per tag"
        self.ctx.use_current_stream()
        pose = state[:, :6].contiguous()
        points, _ = self.ctx.project_points(self.obj if obj is None else obj, pose, self.K, self.dist if self.ndist else None)
        overlay.draw_pose(frames_bgr, draw_frames, points, ok=state[:, H.ST_OK], radius=radius, thickness=thickness)
        return points

    def new_state_buffer(self, frames=1):
        shape = (frames, self.B, H.STATE_STRIDE) if frames > 1 else (self.B, H.STATE_STRIDE)
        return torch.zeros(shape, dtype=torch.float64, device=self.dev)

    def read_state(self):
        """-> list of TrackState (synchronises)."""
        buf = (TrackState * self.B)()
        H.check(self.ctx.L.agt_tracker_state_read(self.ctx.h, C.byref(buf), self.B), "agt_tracker_state_read")
        return list(buf)

    def corners(self):
        """current corner set and LK status as torch views are not exposed by pointer; copy out"""
        cp, sp = C.c_void_p(), C.c_void_p()
        H.check(self.ctx.L.agt_tracker_buffers(self.ctx.h, C.byref(cp), C.byref(sp)), "agt_tracker_buffers")
        return cp.value, sp.value
