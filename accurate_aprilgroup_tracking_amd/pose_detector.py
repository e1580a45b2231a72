"""Host-side mirror of the reference's `PoseDetector`
(/root/reference/aprilgroup_tracking/aprilgroup_pose_estimation/detect_pose.py:28-619),
restricted to the per-frame pose path: model loading (:105-145, :185-227), the
`_estimate_pose` state machine (:467-574) with its motion model (:229-349), and the
north-star LK corner tracking that fills the hole at :573-574.

Every cv2 call goes through `self.cv`, by default the HIP-backed `cv_hip` module, so the
numbers come from the gfx950 kernels; without the HIP library or a GPU construction fails
loudly.  Camera capture and the AprilTag detector itself are out of scope
(SURVEY.md section 2 rows 4-6): a detector is injected as a callable.  Drawing is opt-in
(`draw=True`: the dots of the pose overlay and the tag outlines of the drawing frame, include/agt_draw.h);
without it `_project_draw_points` only records the projected points.

Two backends:

* ``backend="cv"`` (default): every cv2 call of the reference goes through `self.cv` (cv_hip), one
  synchronous host round trip per call -- the literal drop-in for the cv2 module.
* ``backend="stream"``: the reference's per-frame entry point on the DEVICE-RESIDENT path.
  `_detect_and_get_pose(frame)` = one pinned host-to-device copy of the frame -> (BGR: fused
  undistort / gray / crop kernel) -> `agt_track_frame` (LK + solvePnP + gate + motion model, state in HBM) or
  `agt_track_frame_detected` when the injected detector returned >= 2 tags -> one 128-byte device-to-host copy of
  the frame's record.  `extrinsic_guess`, `prev_transform` and the velocity buffers are materialised lazily from
  `agt_tracker_state_read` when somebody looks at them.  `step(raw_frame)` is `process_frame` +
  `_detect_and_get_pose` of the reference's loop (detect_pose.py:669-681) with the raw frame uploaded once.

For many independent streams use `tracker.StreamTracker`, which keeps this same state
machine resident on the device.
"""
import json
from copy import deepcopy
from pathlib import Path

import numpy as np

from .geometry import TransformHelper

OPTFLOW_USE_INITIAL_FLOW = 4        # cv2's value (a cv module handed in need not carry the constant)


class PoseDetector(TransformHelper):
    DIRPATH = 'aprilgroup_tracking/aprilgroup_pose_estimation'
    JSON_FILE = 'april_group.json'

    MIN_TAGS = 2            # detect_pose.py:494
    ERROR_GATE_PX = 2       # detect_pose.py:539
    DECISION_MARGIN = 50    # detect_pose.py:389

    CONSENSUS_MIN = 8       # inliers a tag hypothesis needs to be elected (pnp_consensus_px): more than one tag's own four

    def __init__(self, logger, mtx, dist, enhance_ape, cv=None, detector=None, backend="cv", lk_fb_px=None, pnp_consensus_px=None,
                 lk_predict_px=None, draw=False):
        """`detector(gray) -> iterable of objects with .tag_id, .corners (4,2), .decision_margin`
        stands in for apriltag.Detector(...).detect (detect_pose.py:368-371).
        lk_fb_px: forward-backward check of the LK step (None / 0 = off): a tracked corner whose track back into the previous
        frame ends that many pixels (max norm) or more from where it started is dropped, and with it its tag.  backend
        "stream" hands it to its StreamTracker (fb_check); backend "cv" tracks back with a second calcOpticalFlowPyrLK.
        pnp_consensus_px: tag consensus in front of the pose solve (None / 0 = off): every tag of the frame is solved alone, every
        corner votes on every tag's pose with this reprojection threshold, and only the tags whose four corners all agree with the
        winner go into _estimate_pose (tag_consensus below; the rule: include/agt_hip.h agt_solve_pnp_consensus).  It is NOT
        ERROR_GATE_PX: that gate judges the mean error of the finished solve, this one a single corner under one tag's pose.
        Backend "stream" hands it to its StreamTracker (consensus_px); backend "cv" does it on the host with the cv module.
        lk_predict_px: motion-predicted initial flow of the LK step (None / 0 = off): once the two frames before the one to be tracked
        both gave an accepted pose, the constant-velocity extrapolation of those poses moves the start of every corner's search
        (predict_flow below; the rule: include/agt_hip.h agt_predict_flow); a prediction with a flow beyond this many pixels is not
        trusted and the frame is tracked as ever.  Backend "stream" hands it to its StreamTracker (predict_px); backend "cv" seeds
        calcOpticalFlowPyrLK with OPTFLOW_USE_INITIAL_FLOW.
        draw: the reference's two images of every frame (detect_pose.py:441-465; the rule: include/agt_draw.h): a red dot on every
        projected model corner of an accepted pose, and the tag outlines on a black `self.draw_frame` that is fresh every frame.
        Backend "cv" draws on the host through the `Draw` mirror and the cv module's circle / line, the dots into `self.img` (which
        `self.overlay` then names as well; for a gray frame `self.img` becomes its (g, g, g) copy, so the dots never land in the
        array LK tracks from and the poses are those of draw=False).  Backend "stream" keeps both images on the device: `self.overlay` (the processed colour
        frame with the dots; (g, g, g) for a gray camera) and `self.draw_frame` are cuda u8 (H, W, 3) tensors of the processed frame's
        size, rewritten by every frame on the tracker's stream without a synchronisation of their own, and `self.img` stays the raw
        frame; `_estimate_pose` called with correspondences alone has no frame and draws nothing there.  False (the default): nothing
        is drawn, nothing more is launched and `draw_frame` stays None."""
        TransformHelper.__init__(self, logger, mtx, dist, cv=cv)
        if backend not in ("cv", "stream"):
            raise ValueError("backend must be 'cv' or 'stream'")
        if lk_fb_px is not None and not (np.isfinite(lk_fb_px) and lk_fb_px >= 0):
            raise ValueError("lk_fb_px must be None or a finite threshold >= 0")
        self.backend = backend
        self.lk_fb_px = float(lk_fb_px) if lk_fb_px else None
        if pnp_consensus_px is not None and not (np.isfinite(pnp_consensus_px) and pnp_consensus_px >= 0):
            raise ValueError("pnp_consensus_px must be None or a finite threshold >= 0")
        self.pnp_consensus_px = float(pnp_consensus_px) if pnp_consensus_px else None
        if lk_predict_px is not None and not (np.isfinite(lk_predict_px) and lk_predict_px >= 0):
            raise ValueError("lk_predict_px must be None or a finite threshold >= 0")
        self.lk_predict_px = float(lk_predict_px) if lk_predict_px else None
        self.last_flow_max = None       # backend "cv": flow_max of the latest LK step (0.0 without a prediction, -1.0 when distrusted)
        self._records = 0               # backend "cv": calls of _estimate_pose so far, and the (record index, pose) of the accepted
        self._pose_history = []         # ones among the last two -- what the LK step predicts from
        self.last_consensus = None      # backend "cv": (winning tag's index in the frame's tag list, its inlier count) or None
        self._dev = None                # stream backend: _DeviceStream, created at the first frame (its size fixes the context)
        self.img = None
        self.draw_frame = None
        self.overlay = None
        self.draw = bool(draw)
        self._drawer = None             # backend "cv", draw=True: the Draw mirror on self.cv
        self.prev_transform = (None, None)
        self.extrinsic_guess = (None, None)
        self.rot_velocities = []
        self.tran_velocities = []
        self.enhance_ape = enhance_ape
        self.detector = detector
        self.extrinsics = self.get_extrinsics()
        self.all_objpts = self.get_all_points(self.extrinsics)
        # results of the latest frame (the reference only logs/draws them)
        self.last_pose = (None, None)
        self.last_error = None
        self._pp, self._pp_pending = None, None
        # LK tracking state (north-star): previous gray frame and the corners seen in it
        self._prev_gray = None
        self._prev_corners = None       # (N,2) float32, rows ordered as _prev_ids x 4
        self._prev_ids = None

    # ---- the four attributes _estimate_pose mutates (detect_pose.py:74-83).  backend "cv": plain attributes.  backend
    # "stream": they live in HBM (AgtTrackState) and are read back -- one synchronising 376-byte copy -- only when looked at.
    def _state(self, name):
        if self._dev is not None:
            self._dev.refresh(self)
        return self.__dict__["_st_" + name]

    extrinsic_guess = property(lambda self: self._state("extrinsic_guess"),
                               lambda self, v: self._set_state("extrinsic_guess", v))
    prev_transform = property(lambda self: self._state("prev_transform"),
                              lambda self, v: self._set_state("prev_transform", v))
    rot_velocities = property(lambda self: self._state("rot_velocities"),
                              lambda self, v: self._set_state("rot_velocities", v))
    tran_velocities = property(lambda self: self._state("tran_velocities"),
                               lambda self, v: self._set_state("tran_velocities", v))

    @property
    def projected_points(self):
        """projectPoints(all_objpts) at the latest ACCEPTED pose (detect_pose.py:441-465 minus the drawing).  backend
        "stream" computes it when somebody looks (the drawing is out of scope; the per-frame path does not pay for it)."""
        if self._pp_pending is not None:
            pose, self._pp_pending = self._pp_pending, None
            self._pp, _ = self.cv.projectPoints(self.all_objpts, pose[0], pose[1], self.mtx, self.dist)
        return self._pp

    @projected_points.setter
    def projected_points(self, value):
        self._pp, self._pp_pending = value, None

    def configure_stream(self, width, height):
        """backend "stream": fix the (processed) frame size before the first frame, e.g. to call `_estimate_pose` with
        detector-supplied correspondences only"""
        self._stream().configure(self, width, height)

    def _set_state(self, name, value):
        if self._dev is not None and self._dev.started:
            raise AttributeError("backend='stream': %s lives on the device; reset the detector instead of assigning it" % name)
        self.__dict__["_st_" + name] = value

    @classmethod
    def from_files(cls, logger, camera_params, enhance_ape=True, cv=None, detector=None, april_group=None, backend="cv", lk_fb_px=None,
                   pnp_consensus_px=None, lk_predict_px=None, draw=False):
        """Build from the reference's on-disk files: `CameraParams.npz` (calibrate_camera.py:107-123) and,
        optionally, an `april_group.json` somewhere else than DIRPATH/JSON_FILE (detect_pose.py:54-55).
        `detector` may be a recorded-detections .npz (formats.ReplayDetector) to replay a session."""
        import os
        from . import formats
        mtx, dist, _, _ = formats.load_camera_params(camera_params)
        if isinstance(detector, (str, os.PathLike)):
            detector = formats.ReplayDetector(detector)
        if april_group is None:
            return cls(logger, mtx, dist, enhance_ape, cv=cv, detector=detector, backend=backend, lk_fb_px=lk_fb_px,
                       pnp_consensus_px=pnp_consensus_px, lk_predict_px=lk_predict_px, draw=draw)
        folder, name = os.path.split(os.fspath(april_group))
        sub = type(cls.__name__, (cls,), {"DIRPATH": folder or ".", "JSON_FILE": name})
        return sub(logger, mtx, dist, enhance_ape, cv=cv, detector=detector, backend=backend, lk_fb_px=lk_fb_px,
                   pnp_consensus_px=pnp_consensus_px, lk_predict_px=lk_predict_px, draw=draw)

    # ------------------------------------------------------------------ model (detect_pose.py:105-227)
    def get_extrinsics(self):
        filepath = Path(self.DIRPATH) / self.JSON_FILE
        try:
            with open(filepath, "r") as handle:
                data = json.load(handle)
        except IOError as file_error:
            raise IOError("The filepath: {} does not exist.".format(filepath)) from file_error
        extrinsics = {}
        for key, tag in data['tags'].items():
            tvec = np.array(tag['extrinsics'][:3], dtype=np.float32).reshape((3, 1))
            rvec = np.array(tag['extrinsics'][-3:], dtype=np.float32).reshape((3, 1))
            self.add_values_in_dict(extrinsics, int(key), [tag['size'], tvec, rvec])
        self.logger.info('Successfully Loaded AprilGroup Extrinsics!')
        return extrinsics

    def get_all_points(self, extrinsics):
        if not any(extrinsics):
            raise ValueError("The extrinsic matrix must be supplied.")
        corners = [self.transform_marker_corners(self.get_initial_pts(size), (rvec, tvec))
                   for size, tvec, rvec in (extrinsics[k][:3] for k in extrinsics)]
        self.logger.info('Successfully Obtained Aprilgroup Object Points!')
        return np.array(corners).reshape(-1, 3)

    # ------------------------------------------------------------------ motion model (:229-349)
    def _update_buffers(self, rot_vel, tran_vel, buf_size=2):
        if not np.all(rot_vel) or not np.all(tran_vel):
            raise ValueError("The rotational and translation velocities cannot be empty.")
        self.rot_velocities.append(rot_vel)
        self.tran_velocities.append(tran_vel)
        if len(self.rot_velocities) > buf_size:
            del self.rot_velocities[0]
            del self.tran_velocities[0]

    def get_pose_vel_acc(self, curr_transform, prev_transform):
        prev_rmat = self.cv.Rodrigues(prev_transform[0])[0]
        curr_rmat = self.cv.Rodrigues(curr_transform[0])[0]
        tran_vel = self.get_relative_trans(curr_rmat, curr_transform[1], prev_transform[1])
        rot_vel = self.get_relative_rot(prev_rmat, curr_rmat)
        self._update_buffers(rot_vel, tran_vel)
        if len(self.tran_velocities) < 2:
            return False, tran_vel, rot_vel, 0.0, 0.0
        tran_acc = self.get_relative_trans(self.rot_velocities[-1], self.tran_velocities[-1], self.tran_velocities[-2])
        rot_acc = self.get_relative_rot(self.rot_velocities[-2], self.rot_velocities[-1])
        return True, tran_vel, rot_vel, tran_acc, rot_acc

    def apply_vel_acc(self, transformation, tran_vel, tran_acc, rot_vel, rot_acc):
        half_acc = self.euler_angles_to_rotation_matrix(self.rotation_matrix_to_euler_angles(rot_acc) / 2)
        rmat = self.cv.Rodrigues(transformation[0])[0]
        pose_m = self.get_extrinsic_matrix(rmat, transformation[1])
        vel_m = self.get_extrinsic_matrix(rot_vel, tran_vel)
        acc_m = self.get_extrinsic_matrix(half_acc, 0.5 * tran_acc)
        rmat_pred, tvec_pred = self.get_rmat_tvec(acc_m @ vel_m @ pose_m)
        return self.cv.Rodrigues(rmat_pred)[0], tvec_pred

    # ------------------------------------------------------------------ detection front-end (:351-439)
    def _obtain_detections(self, gray):
        """Same output contract as the reference: lists of (1,4,2) image points, (4,3) object
        points and tag ids for detections with decision_margin >= 50."""
        if self.detector is None:
            raise RuntimeError("no AprilTag detector was injected (the swatbotics detector is out of scope)")
        img_list, obj_list, ids = [], [], []
        if self.mtx is None:
            return img_list, obj_list, ids
        for det in self.detector(gray):
            if det.decision_margin < self.DECISION_MARGIN:
                continue
            size, tvec, rvec = self.extrinsics[det.tag_id][:3]
            img_list.append(np.asarray(det.corners).reshape(1, 4, 2))
            obj_list.append(self.transform_marker_corners(self.get_initial_pts(size), (rvec, tvec)))
            ids.append(det.tag_id)
        return img_list, obj_list, ids

    def _project_draw_points(self, transformation):
        """detect_pose.py:441-465: keeps the projected model corners and, with draw=True, draws them into self.img and
        self.draw_frame (backend "cv"; backend "stream" draws on the device, _DeviceStream._draw)."""
        self.projected_points, _ = self.cv.projectPoints(self.all_objpts, transformation[0], transformation[1],
                                                         self.mtx, self.dist)
        if self.draw and self.img is not None and self.draw_frame is not None:
            if self._drawer is None:
                from .draw import Draw
                self._drawer = Draw(self.logger, cv=self.cv)
            self._drawer.draw_squares_and_3d_pts(self.img, self.draw_frame, self.projected_points)

    # ------------------------------------------------------------------ ★ the state machine (:467-574)
    def _estimate_pose(self, imgpoints_arr, objpoints_arr):
        if self.backend == "stream":
            return self._stream().estimate(self, imgpoints_arr, objpoints_arr)
        prev_snapshot = deepcopy(self.prev_transform)        # solvePnP overwrites aliased guess arrays
        self.last_pose, self.last_error = (None, None), None
        self._records += 1
        if self.pnp_consensus_px and imgpoints_arr and objpoints_arr:
            # tag consensus: the state machine below is unchanged, it sees the tags whose corners all agree with the elected pose
            # (the device: mask = status AND inliers, then the tag gate); no consensus = no tag = the too-few path
            obj = np.array(objpoints_arr, dtype=np.float32).reshape(-1, 3)
            img = np.array(imgpoints_arr, dtype=np.float32).reshape(-1, 2)
            guess = self.extrinsic_guess if (self.extrinsic_guess[0] is not None and self.enhance_ape) else None
            inl, win, cnt, _ = tag_consensus(self.cv, obj, img, self.mtx, self.dist, guess=guess, corners_per_tag=4,
                                             inlier_px=self.pnp_consensus_px, min_inliers=self.CONSENSUS_MIN)
            self.last_consensus = (win, cnt)
            # (the reference solves on whole tags: a tag with a dissenting corner leaves altogether, as under the device's tag gate)
            keep = np.repeat(inl.reshape(-1, 4).all(axis=1), 4)
            ends = np.cumsum([np.asarray(a).reshape(-1, 2).shape[0] for a in imgpoints_arr])
            sel = [bool(keep[e - np.asarray(a).reshape(-1, 2).shape[0]:e].all()) for a, e in zip(imgpoints_arr, ends)]
            imgpoints_arr = [a for a, k in zip(imgpoints_arr, sel) if k]
            objpoints_arr = [a for a, k in zip(objpoints_arr, sel) if k]
        if not (imgpoints_arr and objpoints_arr and len(imgpoints_arr) >= self.MIN_TAGS):
            self.extrinsic_guess = (None, None)
            return
        obj = np.array(objpoints_arr, dtype=np.float32).reshape(-1, 3)
        img = np.array(imgpoints_arr, dtype=np.float32).reshape(-1, 2)
        guided = self.extrinsic_guess[0] is not None and self.enhance_ape
        if guided:
            ok, rvec, tvec = self.cv.solvePnP(obj, img, self.mtx, self.dist, self.extrinsic_guess[0],
                                              self.extrinsic_guess[1], True, flags=self.cv.SOLVEPNP_ITERATIVE)
        else:
            ok, rvec, tvec = self.cv.solvePnP(obj, img, self.mtx, self.dist, flags=self.cv.SOLVEPNP_ITERATIVE)
        if not ok:
            return
        pose = (rvec, tvec)
        self.last_pose = pose
        self.last_error = self.get_reprojection_error(obj, img, pose)
        if not self.last_error < self.ERROR_GATE_PX:
            self.extrinsic_guess = (None, None)
            return
        self._project_draw_points(pose)
        if self.lk_predict_px:
            # (a float64 copy: solvePnP keeps writing into the guess arrays the pose may alias)
            self._pose_history = self._pose_history[-1:] + [(self._records, (np.array(rvec, np.float64).reshape(3, 1),
                                                                               np.array(tvec, np.float64).reshape(3, 1)))]
        if not guided:
            self.extrinsic_guess = pose
        else:
            good, tran_vel, rot_vel, tran_acc, rot_acc = self.get_pose_vel_acc(pose, prev_snapshot)
            if good:
                self.extrinsic_guess = self.apply_vel_acc(prev_snapshot, tran_vel, tran_acc, rot_vel, rot_acc)
        self.prev_transform = pose

    # ------------------------------------------------------------------ per-frame entry (:576-619)
    def undistort_frame(self, frame):
        """detect_pose.py:147-183: optimal new camera matrix (alpha = 1), undistort, crop to the ROI.
        (As in the reference, the ORIGINAL mtx/dist keep being used by solvePnP afterwards.)"""
        height, width = frame.shape[:2]
        new_camera_matrix, roi = self.cv.getOptimalNewCameraMatrix(self.mtx, self.dist, (width, height), 1, (width, height))
        dst = self.cv.undistort(frame, self.mtx, self.dist, None, new_camera_matrix)
        x_val, y_val, width, height = roi
        return dst[y_val:y_val + height, x_val:x_val + width]

    def process_frame(self, frame):
        """detect_pose.py:611-619"""
        if self.dist is not None:
            frame = self.undistort_frame(frame)
        return frame

    def _to_gray(self, frame):
        if frame.ndim == 2:
            return frame
        return self.cv.cvtColor(np.ascontiguousarray(frame), self.cv.COLOR_BGR2GRAY)       # detect_pose.py:602

    def track_corners(self, gray):
        """North-star step: carry the previous frame's corners into `gray` with pyramidal LK
        (21x21 window, 3 levels, COUNT+EPS (30, 0.01)) and return them per tag."""
        seeds, flow, lk_flags = None, None, 0
        if self.lk_predict_px:
            # the frame's record will be number _records + 1: predicted when the two records before it were both accepted
            self.last_flow_max = 0.0
            h = self._pose_history
            if len(h) == 2 and h[0][0] == self._records - 1 and h[1][0] == self._records:
                obj = np.concatenate([self.transform_marker_corners(self.get_initial_pts(self.extrinsics[i][0]), (self.extrinsics[i][2], self.extrinsics[i][1]))
                                      for i in self._prev_ids]).astype(np.float32).reshape(-1, 3)
                seeds, flow, self.last_flow_max, _ = predict_flow(self.cv, obj, self._prev_corners, h[0][1], h[1][1], self.mtx, self.dist,
                                                                  None, self.lk_predict_px)
                lk_flags = OPTFLOW_USE_INITIAL_FLOW
        if seeds is None:
            nxt, status, _ = self.cv.calcOpticalFlowPyrLK(self._prev_gray, gray, self._prev_corners, None, winSize=(21, 21), maxLevel=2)
        else:
            nxt, status, _ = self.cv.calcOpticalFlowPyrLK(self._prev_gray, gray, self._prev_corners, seeds.copy(), winSize=(21, 21), maxLevel=2,
                                                          flags=lk_flags)
        if self.lk_fb_px:
            # forward-backward check (OpenCV's lk_track.py sample): back from where the corners arrived; float32 max norm.  Under
            # lk_predict_px the way back starts at arrival - flow: started at the arrival it would fail as the unseeded forward pass does
            if seeds is None:
                back, st_b, _ = self.cv.calcOpticalFlowPyrLK(gray, self._prev_gray, nxt, None, winSize=(21, 21), maxLevel=2)
            else:
                start = (np.asarray(nxt, np.float32).reshape(-1, 2) - flow).astype(np.float32)
                back, st_b, _ = self.cv.calcOpticalFlowPyrLK(gray, self._prev_gray, np.asarray(nxt, np.float32).reshape(-1, 2), start,
                                                             winSize=(21, 21), maxLevel=2, flags=lk_flags)
            d = np.abs(np.asarray(self._prev_corners, np.float32).reshape(-1, 2) - np.asarray(back, np.float32).reshape(-1, 2)).max(axis=1)
            status = (status.reshape(-1) != 0) & (st_b.reshape(-1) != 0) & (d < np.float32(self.lk_fb_px))
        nxt = nxt.reshape(-1, 4, 2); ok = status.reshape(-1, 4).all(axis=1)
        img_list, obj_list, ids = [], [], []
        for t, tag_id in enumerate(self._prev_ids):
            if not ok[t]:
                continue
            size, tvec, rvec = self.extrinsics[tag_id][:3]
            img_list.append(nxt[t].reshape(1, 4, 2).astype(np.float64))
            obj_list.append(self.transform_marker_corners(self.get_initial_pts(size), (rvec, tvec)))
            ids.append(tag_id)
        return img_list, obj_list, ids

    def frame_buffer(self, shape):
        """backend "stream": a numpy view of PINNED host memory of the given frame shape ((H, W) gray or (H, W, 3) BGR).  A
        capture loop that reads into it (`cap.read(buf)`) and hands it to `_detect_and_get_pose` / `step` saves the host-side
        copy into the staging buffer that any other array costs (about 0.1 ms for a 1280x720 BGR frame)."""
        if self.backend != "stream":
            raise RuntimeError("frame_buffer() belongs to backend='stream'")
        return self._stream().frame_buffer(tuple(shape))

    def _stream(self):
        if self._dev is None:
            self._dev = _DeviceStream(self)
        return self._dev

    def step(self, raw_frame):
        """The body of the reference's capture loop (detect_pose.py:669-681): `frame = self.process_frame(frame)`
        followed by `self._detect_and_get_pose(frame)`.  backend "stream" uploads the RAW frame once and undistorts,
        converts and crops it on the device (no processed frame ever exists on the host; self.img stays the raw frame)."""
        if self.backend == "stream":
            self.img = raw_frame
            return self._stream().frame(self, raw_frame, raw=True)
        return self._detect_and_get_pose(self.process_frame(raw_frame))

    def reset_stream(self):
        """backend "stream": forget pose state and tracked corners (a new sequence); also the recovery from a chain fault"""
        if self._dev is not None:
            self._dev.reset(self)

    def _detect_and_get_pose(self, frame):
        if self.backend == "stream":
            self.img = frame
            return self._stream().frame(self, frame, raw=False)
        self.img = frame
        gray = self._to_gray(frame)
        if self.draw:
            # the dots go into a COLOUR image that is never the LK source: a BGR frame is its own overlay (gray is a cvtColor copy of
            # it, as in the reference); a gray frame IS `gray`, which becomes _prev_gray, so it gets a (g, g, g) copy as on the device
            if frame.ndim == 2:
                self.img = np.repeat(frame[:, :, None], 3, axis=2)
            self.overlay = self.img
            self.draw_frame = np.zeros(frame.shape[:2] + (3,), np.uint8)
        img_list, obj_list, ids = ([], [], [])
        if self.detector is not None:
            img_list, obj_list, ids = self._obtain_detections(gray)
        if len(img_list) < self.MIN_TAGS and self._prev_gray is not None and self._prev_ids:
            img_list, obj_list, ids = self.track_corners(gray)      # fills detect_pose.py:573-574
        self._estimate_pose(img_list, obj_list)
        if ids:
            self._prev_gray = gray
            self._prev_corners = np.array(img_list, dtype=np.float32).reshape(-1, 2)
            self._prev_ids = list(ids)


def predict_flow(cv, obj, prev_pts, older, newer, mtx, dist, usable, max_flow_px):
    """The seed rule of the motion-predicted initial flow (include/agt_hip.h agt_predict_flow) on the host, with the `cv` module's
    Rodrigues / projectPoints: obj (n,3), prev_pts (n,2) float32 (the corners in the newer frame), older / newer = (rvec, tvec) of the two
    frames before the one to be tracked, usable (n,) bool or None.
    -> (seeds (n,2) float32, flow (n,2) float32, flow_max: 0.0 without usable corners, -1.0 when the prediction is not trusted (the seeds
    are then prev_pts bit for bit), (rvec, tvec) of the predicted pose)."""
    if not (np.isfinite(max_flow_px) and max_flow_px > 0):
        raise ValueError("predict_flow: a finite max_flow_px > 0 is expected")
    prev = np.ascontiguousarray(np.asarray(prev_pts, np.float32).reshape(-1, 2))
    n = prev.shape[0]
    obj64 = np.asarray(obj).reshape(n, 3).astype(np.float64)
    usable = np.ones(n, bool) if usable is None else np.asarray(usable).reshape(n) != 0
    r2, t2 = (np.asarray(v, np.float64).reshape(3, 1) for v in older)
    r1, t1 = (np.asarray(v, np.float64).reshape(3, 1) for v in newer)
    nothing = (prev.copy(), np.zeros((n, 2), np.float32), -1.0)
    nan_pose = (np.full((3, 1), np.nan), np.full((3, 1), np.nan))
    if not all(np.isfinite(v).all() for v in (r2, t2, r1, t1)):
        return nothing + (nan_pose,)
    R2 = np.asarray(cv.Rodrigues(r2)[0], np.float64).reshape(3, 3)
    R1 = np.asarray(cv.Rodrigues(r1)[0], np.float64).reshape(3, 3)
    D = R1 @ R2.T                       # the camera-frame motion older -> newer, applied once more
    Rp = D @ R1
    tp = D @ (t1 - t2) + t1
    rp = np.asarray(cv.Rodrigues(Rp)[0], np.float64).reshape(3, 1)
    pred = (rp, tp)
    p1, _ = cv.projectPoints(obj64, r1, t1, mtx, dist)
    pp, _ = cv.projectPoints(obj64, rp, tp, mtx, dist)
    with np.errstate(over="ignore", invalid="ignore"):
        flow = (np.asarray(pp, np.float64).reshape(n, 2) - np.asarray(p1, np.float64).reshape(n, 2)).astype(np.float32)
    Rpp = np.asarray(cv.Rodrigues(rp)[0], np.float64).reshape(3, 3)
    z1 = obj64 @ R1[2] + t1[2, 0]
    zp = obj64 @ Rpp[2] + tp[2, 0]
    mag = np.abs(flow).max(axis=1) if n else np.zeros(0, np.float32)
    with np.errstate(invalid="ignore"):
        fine = (z1 > 0.0) & (zp > 0.0) & np.isfinite(flow).all(axis=1) & (mag <= np.float32(max_flow_px))
    if not fine[usable].all():
        return nothing + (pred,)
    flow[~usable] = 0.0
    seeds = prev.copy()
    seeds[usable] = prev[usable] + flow[usable]          # (float32 add per component)
    return seeds, flow, float(mag[usable].max()) if usable.any() else 0.0, pred


def tag_consensus(cv, obj, img, mtx, dist, usable=None, guess=None, corners_per_tag=4, inlier_px=2.0, min_inliers=8):
    """The tag-consensus rule (include/agt_hip.h agt_solve_pnp_consensus, steps 1 - 5) on the host, with the `cv` module's solvePnP /
    projectPoints / Rodrigues: obj (n,3), img (n,2), tag t = rows corners_per_tag * t ..; usable (n,) bool or None; guess (rvec, tvec) or
    None -- every hypothesis starts from a float64 COPY of it (solvePnP writes into its guess arrays).
    -> (inliers (n,) bool, winning tag or -1, its inlier count or 0, the winner's (rvec, tvec) or None)."""
    cpt = int(corners_per_tag)
    n = obj.shape[0]
    if cpt < 4 or n == 0 or n % cpt or min_inliers < cpt or not (np.isfinite(inlier_px) and inlier_px > 0):
        raise ValueError("tag_consensus: whole tags of >= 4 corners, min_inliers >= corners_per_tag and a finite inlier_px > 0 are expected")
    usable = np.ones(n, bool) if usable is None else np.asarray(usable).reshape(n) != 0
    img64 = np.asarray(img, np.float64).reshape(n, 2)
    obj64 = np.asarray(obj, np.float64).reshape(n, 3)
    tau2 = float(inlier_px) * float(inlier_px)
    best = (-1, -1, 0.0, None, None)
    for t in range(n // cpt):
        sl = slice(t * cpt, (t + 1) * cpt)
        if not usable[sl].all():
            continue
        try:
            if guess is not None:
                ok, r, tv = cv.solvePnP(obj[sl], img[sl], mtx, dist, np.array(guess[0], np.float64).reshape(3, 1),
                                        np.array(guess[1], np.float64).reshape(3, 1), True, flags=cv.SOLVEPNP_ITERATIVE)
            else:
                ok, r, tv = cv.solvePnP(obj[sl], img[sl], mtx, dist, flags=cv.SOLVEPNP_ITERATIVE)
        except ValueError:          # (a solver that reports too few points / a singular system by raising)
            continue
        r = np.asarray(r, np.float64).reshape(3); tv = np.asarray(tv, np.float64).reshape(3)
        if not ok or not (np.isfinite(r).all() and np.isfinite(tv).all()):
            continue
        proj, _ = cv.projectPoints(obj64, r.reshape(3, 1), tv.reshape(3, 1), mtx, dist)
        d = np.asarray(proj, np.float64).reshape(n, 2) - img64
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        R = np.asarray(cv.Rodrigues(r.reshape(3, 1))[0], np.float64).reshape(3, 3)
        zc = obj64 @ R[2] + tv[2]
        with np.errstate(invalid="ignore"):
            inl = usable & (zc > 0.0) & (d2 < tau2)
        cnt, ssq = int(inl.sum()), float(d2[inl].sum())
        if best[0] < 0 or cnt > best[1] or (cnt == best[1] and ssq < best[2]):
            best = (t, cnt, ssq, inl, (r.reshape(3, 1), tv.reshape(3, 1)))
    if best[0] < 0 or best[1] < min_inliers:
        return np.zeros(n, bool), -1, 0, None
    return best[3], best[0], best[1], best[4]


class _DeviceStream:
    """backend "stream" of PoseDetector: one stream of tracker.StreamTracker plus the pinned staging buffers of the three
    copies a frame costs (frame up, corner table up when the detector spoke, 128-byte record down)."""

    def __init__(self, det):
        import ctypes as C
        import torch
        from . import hiplib as H
        from . import cv_hip
        cv_hip._require_gpu()
        self.C, self.torch, self.H = C, torch, H
        self.trk = None
        self.started = False
        self.n = det.all_objpts.shape[0]
        self.tag_ids = list(det.extrinsics)
        obj32 = det.all_objpts.astype(np.float32)
        # a detection's object points are the float32-identical rows of all_objpts: recognise the tag by them
        self.tag_of = {np.ascontiguousarray(obj32[4 * t:4 * t + 4]).tobytes(): t for t in range(self.n // 4)}
        self.dirty = False
        self.has_prev = False
        self.shape = None
        self._pin = {}                  # frame_buffer(): pinned arrays handed to the caller (the capture writes into them)
        self._stage = {}                # pinned staging of frames that live anywhere else (never the caller's buffers)
        self.roi = None
        self.draw = det.draw
        self.ov_raw = None              # draw=True: the uploaded colour frame, the overlay (a view of it, or of its undistorted copy)
        self.ov, self.draw_t = None, None       # and the drawing frame, all made at the first frame

    # ---- set-up at the first frame
    def _setup(self, det, shape, raw):
        torch, H = self.torch, self.H
        from .tracker import StreamTracker
        h, w = shape[:2]
        self.src_hw = (h, w)
        self.undistort = bool(raw and det.dist is not None)
        if self.undistort:
            new_k, roi = det.cv.getOptimalNewCameraMatrix(det.mtx, det.dist, (w, h), 1, (w, h))
            self.roi = roi
            gw, gh = roi[2], roi[3]
        else:
            new_k, self.roi, gw, gh = None, (0, 0, w, h), w, h
        self.trk = StreamTracker(gw, gh, det.all_objpts, det.mtx, det.dist, n_streams=1, max_level=2, win=21,
                                 enhance_ape=det.enhance_ape, reproject=False, min_points=4 * det.MIN_TAGS,
                                 gate_px=float(det.ERROR_GATE_PX), fb_check=det.lk_fb_px or 0.0,
                                 consensus_px=det.pnp_consensus_px or 0.0, consensus_min=det.CONSENSUS_MIN,
                                 predict_px=det.lk_predict_px or 0.0)
        self.trk.tag_gate(4)
        self.trk.pipeline(1)
        self.trk.reset()
        ctx = self.trk.ctx
        if self.undistort:
            ctx.undistort_init(det.mtx, det.dist, new_k, w, h)
        dev = self.trk.dev
        self.gpitch = (gw + 15) & ~15
        self.gray = [torch.zeros((1, gh, self.gpitch), dtype=torch.uint8, device=dev) for _ in range(4)]
        self.gi = 0
        self.bgr = None
        self.table_host = torch.zeros(self.n * 9, dtype=torch.uint8).pin_memory()
        self.table_dev = torch.zeros(self.n * 9, dtype=torch.uint8, device=dev)
        self.rec_host = torch.zeros(H.STATE_STRIDE, dtype=torch.float64).pin_memory()
        self.rec_np = self.rec_host.numpy()
        self.rec_dev = torch.zeros((1, H.STATE_STRIDE), dtype=torch.float64, device=dev)
        self.pts_np = self.table_host.numpy()[:self.n * 8].view(np.float32).reshape(self.n, 2)
        self.mask_np = self.table_host.numpy()[self.n * 8:]
        self.gw, self.gh = gw, gh
        self.shape = tuple(shape)
        self.raw = raw

    def frame_buffer(self, shape):
        buf = self._pin.get(shape)
        if buf is None:
            buf = self._pin[shape] = self.torch.zeros(shape, dtype=self.torch.uint8).pin_memory()
        return buf.numpy()

    def _pinned(self, frame):
        """-> pinned tensor holding `frame`: the caller's own frame_buffer() when the frame IS that buffer, otherwise a
        staging buffer of this object (a caller's capture buffer is never overwritten)"""
        t = self._pin.get(frame.shape)
        if t is not None and frame.ctypes.data == t.data_ptr() and frame.flags.c_contiguous:
            return t
        t = self._stage.get(frame.shape)
        if t is None:
            t = self._stage[frame.shape] = self.torch.zeros(frame.shape, dtype=self.torch.uint8).pin_memory()
        np.copyto(t.numpy(), frame)
        return t

    def _gray_as_bgr(self, frame):
        """a GRAY raw frame of a camera with lens distortion (process_frame undistorts whatever it gets, detect_pose.py:611-619):
        staged as three equal channels and sent down the BGR path -- remap acts per channel and BGR2GRAY of (g, g, g) is g
        ((1868 + 9617 + 4899) g + 2^13 >> 14), so the result is cv.undistort(gray) cropped to the ROI, byte for byte"""
        shape = frame.shape + (3,)
        t = self._stage.get(shape)
        if t is None:
            t = self._stage[shape] = self.torch.zeros(shape, dtype=self.torch.uint8).pin_memory()
        np.copyto(t.numpy(), frame[:, :, None])
        return t

    def _overlay_source(self, det, pin, staged):
        """draw=True: where this frame's colour image for det.overlay comes from.  staged: the frame's own upload puts it into
        self.bgr (every BGR or (g, g, g) frame of _ingest; the one-call path when it undistorts, which copies first): nothing more is
        uploaded and _draw reads self.bgr.  Otherwise -- a gray frame that is not undistorted, a BGR frame the one-call path reads
        from pinned memory directly -- `pin` is uploaded once more into ov_raw ((g, g, g) for a gray one), BEFORE the frame is tracked:
        the copy has left `pin` when the frame's record arrives."""
        torch = self.torch
        if self.ov_raw is None:
            h, w = self.src_hw
            dev = self.trk.dev
            self.ov_raw = torch.zeros((1, h, w, 3), dtype=torch.uint8, device=dev)
            self.ov_gray = torch.zeros((h, w), dtype=torch.uint8, device=dev)
            self.draw_t = torch.zeros((1, self.gh, self.gw, 3), dtype=torch.uint8, device=dev)
            obj = np.asarray(det.all_objpts)
            self.obj_draw = torch.from_numpy(np.ascontiguousarray(obj.reshape(-1, 3), dtype=np.float32 if obj.dtype == np.float32 else np.float64)).to(dev)
        self.ov_staged = staged
        if staged:
            return
        if pin.dim() == 2:
            self.ov_gray.copy_(pin, non_blocking=True)
            self.ov_raw[0].copy_(self.ov_gray.unsqueeze(2).expand(-1, -1, 3))
        else:
            self.ov_raw[0].copy_(pin, non_blocking=True)

    def _draw(self, det):
        """draw=True: the overlay -- a tensor of its own, never the staging buffer: the undistorted copy of the colour frame cropped to
        the ROI as a view, or ov_raw (a device-to-device copy of self.bgr when the frame was staged there) -- then dots into it and
        outlines onto the cleared drawing frame, at the pose of the record in rec_dev and only if it was accepted; enqueued behind the
        frame's own work, nothing is read back"""
        if self.undistort:
            x, y, w, h = self.roi
            self.ov = self.trk.ctx.undistort_bgr(self.bgr if self.ov_staged else self.ov_raw)[:, y:y + h, x:x + w]
        else:
            if self.ov_staged:
                self.ov_raw.copy_(self.bgr)
            self.ov = self.ov_raw
        self.trk.draw_overlay(self.ov, self.draw_t, self.rec_dev, obj=self.obj_draw)
        det.overlay, det.draw_frame = self.ov[0], self.draw_t[0]

    def _upload(self, dst, src_t, nbytes):
        ctx = self.trk.ctx
        self.H.check(ctx.L.agt_upload(ctx.h, self.C.c_void_p(dst.data_ptr()), self.C.c_void_p(src_t.data_ptr()), nbytes), "agt_upload")

    def _ingest(self, det, frame, raw):
        """frame (host) -> gray frame in HBM (one of four rotating buffers: the previous frame stays valid for LK)"""
        torch = self.torch
        frame = np.asarray(frame)
        if frame.dtype != np.uint8 or frame.ndim not in (2, 3) or (frame.ndim == 3 and frame.shape[2] != 3):
            raise ValueError("an 8-bit gray (H, W) or BGR (H, W, 3) frame is expected")
        if self.trk is None:
            self._setup(det, frame.shape, raw)
        elif tuple(frame.shape) != self.shape or raw != self.raw:
            raise ValueError("backend='stream': frame shape / kind changed from %r to %r; use a new detector" % (self.shape, frame.shape))
        ctx = self.trk.ctx
        ctx.use_current_stream()
        self.gi = (self.gi + 1) & 3
        g = self.gray[self.gi]
        if frame.ndim == 2 and not self.undistort:
            assert frame.shape == (self.gh, self.gw)
            pin = self._pinned(frame)
            if self.draw:
                self._overlay_source(det, pin, staged=False)
            if self.gpitch == self.gw:
                self._upload(g, pin, frame.size)
            else:       # pitch-padded rows: 2-D copy through torch (rare: widths that are not a multiple of 16)
                g[0, :, :self.gw].copy_(pin, non_blocking=True)
            return g[:, :, :self.gw]
        pin = self._gray_as_bgr(frame) if frame.ndim == 2 else self._pinned(frame)
        if self.draw:
            self._overlay_source(det, pin, staged=True)
        if self.bgr is None:
            self.bgr = torch.zeros((1,) + tuple(pin.shape), dtype=torch.uint8, device=self.trk.dev)
        self._upload(self.bgr, pin, pin.numel())
        ctx.preprocess_bgr(self.bgr, self.roi, undistort=self.undistort, out=g[:, :, :self.gw])
        return g[:, :, :self.gw]

    # ---- per-frame entry
    def frame(self, det, frame, raw):
        if det.detector is None and self.has_prev and self.trk is not None:
            return self._frame_tracked_one_call(det, frame, raw)
        g = self._ingest(det, frame, raw)
        img_list, obj_list, ids = [], [], []
        if det.detector is not None:
            gray_host = frame if (np.ndim(frame) == 2 and not self.undistort) else g[0].cpu().numpy()     # the PROCESSED frame
            img_list, obj_list, ids = det._obtain_detections(gray_host)
        if len(img_list) >= det.MIN_TAGS or not self.has_prev:
            self._table(img_list, obj_list)
            self._upload(self.table_dev, self.table_host, self.n * 9)
            pts = self.table_dev[:self.n * 8].view(self.torch.float32).view(1, self.n, 2)
            mask = self.table_dev[self.n * 8:].view(1, self.n)
            self.trk.step_detected(g, pts, mask, self.rec_dev)
            self.has_prev = self.has_prev or bool(ids)      # (the mirror's `if ids:`: a frame without any tag is no tracking source)
            if self.draw:
                self._draw(det)
            self._finish(det)
        else:
            self.trk.step(g, self.rec_dev)        # LK from the previous frame's corners: fills detect_pose.py:573-574
            self.trk.join()
            if self.draw:
                self._draw(det)
            self._finish(det, tracked=True)

    def _frame_tracked_one_call(self, det, frame, raw):
        """LK path without a detector: upload, pre-processing, agt_track_frame, join, record download and the wait in ONE
        foreign call (agt_track_host_frame)"""
        frame = np.asarray(frame)
        if tuple(frame.shape) != self.shape or raw != self.raw or frame.dtype != np.uint8:
            raise ValueError("backend='stream': frame shape / kind changed from %r to %r; use a new detector" % (self.shape, frame.shape))
        C, ctx = self.C, self.trk.ctx
        ctx.use_current_stream()
        self.gi = (self.gi + 1) & 3
        g = self.gray[self.gi]
        color = frame.ndim == 3 or self.undistort          # a gray raw frame that must be undistorted travels as (g, g, g)
        pin = self._gray_as_bgr(frame) if (color and frame.ndim == 2) else self._pinned(frame)
        if color and self.bgr is None:
            self.bgr = self.torch.zeros((1,) + tuple(pin.shape), dtype=self.torch.uint8, device=self.trk.dev)
        if self.draw:
            self._overlay_source(det, pin, staged=bool(color and self.undistort))
        self.H.check(ctx.L.agt_track_host_frame(ctx.h, C.c_void_p(pin.data_ptr()), 3 if color else 1, self.src_hw[1], self.src_hw[0],
                                                C.c_void_p(self.bgr.data_ptr()) if color else None, int(self.undistort and color),
                                                self.roi[0] if color else 0, self.roi[1] if color else 0, C.c_void_p(g.data_ptr()), self.gpitch,
                                                # (no device copy of the record, it arrives in host memory, polled -- unless the drawing reads it)
                                                C.c_void_p(self.rec_dev.data_ptr()) if self.draw else None,
                                                C.c_void_p(self.rec_host.data_ptr())), "agt_track_host_frame")
        if self.draw:
            self._draw(det)
        self.trk._alive.append(g)
        if len(self.trk._alive) > self.trk._keep_frames:
            del self.trk._alive[0]
        self._finish(det, downloaded=True, tracked=True)

    def estimate(self, det, imgpoints_arr, objpoints_arr):
        """_estimate_pose(img_list, obj_list) with caller-supplied correspondences (no frame)"""
        if self.trk is None:
            raise RuntimeError("backend='stream': _estimate_pose needs the frame size; call configure(width, height) or feed a frame first")
        self.trk.ctx.use_current_stream()
        self._table(imgpoints_arr or [], objpoints_arr or [])
        self._upload(self.table_dev, self.table_host, self.n * 9)
        pts = self.table_dev[:self.n * 8].view(self.torch.float32).view(1, self.n, 2)
        mask = self.table_dev[self.n * 8:].view(1, self.n)
        self.trk.estimate_pose(pts, mask, self.rec_dev)
        self._finish(det)

    def configure(self, det, width, height):
        if self.trk is None:
            self._setup(det, (height, width), False)

    def _table(self, img_list, obj_list):
        self.pts_np[:] = 0.0
        self.mask_np[:] = 0
        for img, obj in zip(img_list, obj_list):
            t = self.tag_of.get(np.ascontiguousarray(np.asarray(obj, np.float32).reshape(4, 3)).tobytes())
            if t is None:
                raise ValueError("backend='stream': object points that are not a tag of april_group.json")
            self.pts_np[4 * t:4 * t + 4] = np.asarray(img, np.float32).reshape(4, 2)
            self.mask_np[4 * t:4 * t + 4] = 1

    def _finish(self, det, downloaded=False, tracked=False):
        H = self.H
        ctx = self.trk.ctx
        if not downloaded:
            H.check(ctx.L.agt_download(ctx.h, self.C.c_void_p(self.rec_host.data_ptr()), self.C.c_void_p(self.rec_dev.data_ptr()),
                                       8 * H.STATE_STRIDE), "agt_download")
        self.started = True
        self.dirty = True
        r = self.rec_np
        flags = int(r[H.ST_FLAGS])
        if tracked and int(r[H.ST_NTRACK]) == 0 and not (flags & H.TRK_CHAIN_TIMEOUT):
            # LK lost every tag: the reference (and the mirror's `if ids:`) keeps the OLDER frame as "previous" and tracks the next
            # frame from it (detect_pose.py:570-574).  The frame is taken back; its gray buffer is the next frame's.
            self.trk.rewind()
            self.gi = (self.gi - 1) & 3
        if flags & H.TRK_CHAIN_TIMEOUT:
            raise RuntimeError("backend='stream': the chained launch gave up waiting for this frame's corners; call reset_stream()")
        if flags & H.PNP_TOO_FEW:
            det.last_pose, det.last_error = (None, None), None
            return
        tdt = np.float32 if r[H.ST_TVEC_F32] else np.float64
        det.last_pose = (r[0:3].reshape(3, 1).copy(), r[3:6].astype(tdt).reshape(3, 1))
        det.last_error = float(r[H.ST_ERR])
        if r[H.ST_OK]:
            det._pp_pending = det.last_pose
        if flags & H.TRK_ZERO_VELOCITY:
            raise ValueError("The rotational and translation velocities cannot be empty.")      # detect_pose.py:236-237

    def refresh(self, det):
        """device tracker state -> the reference's attributes (only when somebody looks)"""
        if not self.dirty:
            return
        self.dirty = False
        s = self.trk.read_state()[0]
        d = det.__dict__
        if s.has_guess:
            g = np.array(s.guess[:])
            d["_st_extrinsic_guess"] = (g[:3].reshape(3, 1), g[3:].astype(np.float32 if s.guess_t_f32 else np.float64).reshape(3, 1))
        else:
            d["_st_extrinsic_guess"] = (None, None)
        if s.has_prev:
            p = np.array(s.prev[:])
            d["_st_prev_transform"] = (p[:3].reshape(3, 1), p[3:].astype(np.float32 if s.prev_t_f32 else np.float64).reshape(3, 1))
        else:
            d["_st_prev_transform"] = (None, None)
        d["_st_rot_velocities"] = [np.array(s.rot_vel[i][:]).reshape(3, 3) for i in range(s.n_vel)]
        d["_st_tran_velocities"] = [np.array(s.tran_vel[i][:]).reshape(3, 1) for i in range(s.n_vel)]

    def reset(self, det):
        if self.trk is not None:
            self.trk.reset()
        self.has_prev = False
        self.started = False
        d = det.__dict__
        d["_st_extrinsic_guess"] = (None, None); d["_st_prev_transform"] = (None, None)
        d["_st_rot_velocities"] = []; d["_st_tran_velocities"] = []
        self.dirty = False
