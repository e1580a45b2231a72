"""ctypes binding of the dense-model library (include/agt_model.h -> libagt_model.so).
Built by build() of __graft_entry__ and loaded by _sidelib.load under the rules of hiplib: there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import _addr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagt_model.so")

VERSION = 100
OK = 0
ERR_ARG, ERR_ALLOC, ERR_CAMERA, ERR_HIP, ERR_ORDER = -1, -2, -3, -5, -12
ERRORS = {ERR_ARG: "ARG", ERR_ALLOC: "ALLOC", ERR_CAMERA: "CAMERA", ERR_HIP: "HIP", ERR_ORDER: "ORDER"}
MAX_TAGS, MAX_SAMPLES, MAX_SIZE, MAX_COUNT = 256, 4194304, 16384, 4096

# every symbol include/agt_model.h declares
SYMBOLS = ["agt_model_version", "agt_dense_model_create", "agt_dense_model_destroy", "agt_dense_model_begin_pass",
           "agt_dense_model_accumulate", "agt_dense_model_read"]


class Problem(C.Structure):
    _fields_ = [("K", C.c_void_p), ("dist", C.c_void_p), ("ndist", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("n_tags", C.c_int32), ("tag_corners", C.c_void_p), ("n_samples", C.c_int32), ("facing", C.c_int32),
                ("model_xyz", C.c_void_p), ("sample_tag", C.c_void_p), ("max_view_deg", C.c_double)]


class ModelError(_sidelib.SideLibError):
    """A call of libagt_model.so returned a negative code."""
    PREFIX, ERRORS = "MODEL", ERRORS


def _declare(L):
    vp, f64, sz = C.c_void_p, C.c_double, C.c_size_t
    L.agt_model_version.restype = C.c_int
    L.agt_dense_model_create.argtypes = [C.POINTER(Problem), vp, C.POINTER(vp)]
    L.agt_dense_model_destroy.argtypes = [vp]
    L.agt_dense_model_begin_pass.argtypes = [vp, f64, f64]
    L.agt_dense_model_accumulate.argtypes = [vp, vp, sz, sz, C.c_int, vp, vp, vp]
    L.agt_dense_model_read.argtypes = [vp, vp, vp, vp, vp]


_lib = None


def lib():
    """Load libagt_model.so (once).  Raises RuntimeError when it is missing."""
    global _lib
    if _lib is None:
        _lib = _sidelib.load(LIB_PATH, _declare)
    return _lib


check = ModelError.check


class DenseModelHandle(_sidelib.Handle):
    """One agt_dense_model handle: a problem checked and uploaded once.  tag_corners (T, 4, 3) f32, model_xyz (M, 3) f32, sample_tag (M,) i32."""
    DESTROY = "agt_dense_model_destroy"

    def __init__(self, cameraMatrix, distCoeffs, width, height, tag_corners, model_xyz, sample_tag, max_view_deg=60.0, facing=1, stream=None):
        self.L = lib()
        K = np.ascontiguousarray(np.asarray(cameraMatrix, np.float64).reshape(3, 3))
        dist = None if distCoeffs is None else np.ascontiguousarray(np.asarray(distCoeffs, np.float64).reshape(-1))
        tc = np.ascontiguousarray(np.asarray(tag_corners, np.float32).reshape(-1, 4, 3))
        xyz = np.ascontiguousarray(np.asarray(model_xyz, np.float32).reshape(-1, 3))
        tag = np.ascontiguousarray(np.asarray(sample_tag, np.int32).reshape(-1))
        if tag.size != xyz.shape[0]:
            raise ValueError("dense model: %d samples, %d tag indices" % (xyz.shape[0], tag.size))
        self.T, self.M, self.width, self.height = int(tc.shape[0]), int(xyz.shape[0]), int(width), int(height)
        p = Problem(_addr(K), None if dist is None or dist.size == 0 else _addr(dist), 0 if dist is None else int(dist.size),
                    self.width, self.height, self.T, _addr(tc), self.M, int(facing), _addr(xyz), _addr(tag), float(max_view_deg))
        self.h = C.c_void_p()
        check(self.L.agt_dense_model_create(C.byref(p), C.c_void_p(stream) if stream else None, C.byref(self.h)), "agt_dense_model_create")

    def begin_pass(self, clip_sigma=0.0, sigma_floor=0.0):
        check(self.L.agt_dense_model_begin_pass(self.h, float(clip_sigma), float(sigma_floor)), "agt_dense_model_begin_pass")

    def accumulate(self, frames_ptr, pitch, frame_stride, count, poses, use=None):
        """frames_ptr: device address; poses (count, 6) f64 host; use (count,) u8 host or None -> frame_obs (count,) i32"""
        poses = np.ascontiguousarray(np.asarray(poses, np.float64).reshape(-1, 6))
        if poses.shape[0] != count:
            raise ValueError("accumulate: %d frames, %d poses" % (count, poses.shape[0]))
        if use is not None:
            use = np.ascontiguousarray(np.asarray(use).reshape(-1) != 0).astype(np.uint8)
            if use.size != count:
                raise ValueError("accumulate: %d frames, %d use bytes" % (count, use.size))
        obs = np.zeros(max(int(count), 0), np.int32)
        check(self.L.agt_dense_model_accumulate(self.h, C.c_void_p(frames_ptr), int(pitch), int(frame_stride), int(count), _addr(poses),
                                                None if use is None else _addr(use), _addr(obs) if obs.size else None),
              "agt_dense_model_accumulate")
        return obs

    def read(self):
        """-> (n i32, S f64, S2 f64, rejected i32), each (M,): the current pass's raw sums"""
        n, rej = np.zeros(self.M, np.int32), np.zeros(self.M, np.int32)
        S, S2 = np.zeros(self.M, np.float64), np.zeros(self.M, np.float64)
        check(self.L.agt_dense_model_read(self.h, _addr(n), _addr(S), _addr(S2), _addr(rej)), "agt_dense_model_read")
        return n, S, S2, rej
