"""ctypes binding of the offline camera calibration library (include/agt_camcal.h -> libagt_camcal.so).
Built by build() of __graft_entry__ and loaded by _sidelib.load under the rules of hiplib: there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import (Options, Report, STOP_CONVERGED, STOP_MAX_ITERS, STOP_LAMBDA, STOP_NAMES,  # noqa: F401
                       _f64, _addr)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagt_camcal.so")

VERSION = 100
OK = 0
ERR_ARG, ERR_ALLOC, ERR_CAMERA, ERR_HIP, ERR_TOO_FEW, ERR_SINGULAR, ERR_DEGENERATE = -1, -2, -3, -5, -10, -11, -12
ERRORS = {ERR_ARG: "ARG", ERR_ALLOC: "ALLOC", ERR_CAMERA: "CAMERA", ERR_HIP: "HIP", ERR_TOO_FEW: "TOO_FEW", ERR_SINGULAR: "SINGULAR",
          ERR_DEGENERATE: "DEGENERATE"}
MAX_VIEWS, MIN_VIEW_POINTS, MAX_VIEW_POINTS, NCAM = 65536, 4, 4096, 16
# the camera vector c[16]
CAMERA_NAMES = ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6", "s1", "s2", "s3", "s4"]

# every symbol include/agt_camcal.h declares
SYMBOLS = ["agt_camcal_version", "agt_camcal_create", "agt_camcal_destroy", "agt_camcal_eval", "agt_camcal_step",
           "agt_camcal_default_options", "agt_camcal_solve"]


class Problem(C.Structure):
    _fields_ = [("n_views", C.c_int32), ("ndist", C.c_int32), ("free_mask", C.c_uint32), ("reserved0", C.c_int32),
                ("view_start", C.c_void_p), ("object_points", C.c_void_p), ("image_points", C.c_void_p)]


class CamCalError(_sidelib.SideLibError):
    """A call of libagt_camcal.so returned a negative code (or camera_calib refused the problem with one)."""
    PREFIX, ERRORS = "CAMCAL", ERRORS


def _declare(L):
    vp, f64 = C.c_void_p, C.c_double
    L.agt_camcal_version.restype = C.c_int
    L.agt_camcal_create.argtypes = [C.POINTER(Problem), vp, C.POINTER(vp)]
    L.agt_camcal_destroy.argtypes = [vp]
    L.agt_camcal_eval.argtypes = [vp, vp, vp, vp, C.POINTER(f64)]
    L.agt_camcal_step.argtypes = [vp, f64, vp, vp, vp, vp]
    L.agt_camcal_default_options.argtypes = [C.POINTER(Options)]
    L.agt_camcal_solve.argtypes = [vp, C.POINTER(Options), vp, vp, C.POINTER(Report)]


_lib = None


def lib():
    """Load libagt_camcal.so (once).  Raises RuntimeError when it is missing."""
    global _lib
    if _lib is None:
        _lib = _sidelib.load(LIB_PATH, _declare)
    return _lib


check = CamCalError.check


def pack_views(object_points, image_points):
    """lists of per-view (n_v, 3) / (n_v, 2) arrays -> (view_start (V + 1,) i32, X (N, 3) f64, img (N, 2) f64)"""
    obj = [_f64(o, (-1, 3)) for o in object_points]
    img = [_f64(i, (-1, 2)) for i in image_points]
    if len(obj) != len(img) or any(len(o) != len(i) for o, i in zip(obj, img)):
        raise ValueError("object and image points: the views do not match")
    start = np.zeros(len(obj) + 1, np.int32)
    start[1:] = np.cumsum([len(o) for o in obj])
    X = np.concatenate(obj) if obj else np.zeros((0, 3))
    m = np.concatenate(img) if img else np.zeros((0, 2))
    return start, np.ascontiguousarray(X), np.ascontiguousarray(m)


class CamCal(_sidelib.Handle):
    """One agt_camcal handle: a problem checked and uploaded once.

    object_points / image_points: lists of per-view (n_v, 3) / (n_v, 2); free_mask: bit i = entry i of the camera vector
    (CAMERA_NAMES) is estimated; ndist: 0, 4, 5, 8 or 12.  camera is (16,), view poses are (V, 6) rvec | tvec."""
    DESTROY = "agt_camcal_destroy"

    def __init__(self, object_points, image_points, free_mask, ndist, stream=None):
        self.L = lib()
        start, X, m = pack_views(object_points, image_points)
        self.V, self.N = len(start) - 1, int(start[-1])
        p = Problem(self.V, int(ndist), int(free_mask), 0, _addr(start), _addr(X), _addr(m))
        self.h = C.c_void_p()
        check(self.L.agt_camcal_create(C.byref(p), C.c_void_p(stream) if stream else None, C.byref(self.h)), "agt_camcal_create")

    def eval(self, camera, view_poses):
        """-> (residuals (N, 2) in the caller's point order, cost)"""
        c, vp = _f64(camera, (NCAM,)), _f64(view_poses, (self.V, 6))
        res = np.zeros((self.N, 2), np.float64)
        cost = C.c_double()
        check(self.L.agt_camcal_eval(self.h, _addr(c), _addr(vp), _addr(res), C.byref(cost)), "agt_camcal_eval")
        return res, cost.value

    def step(self, lam, camera, view_poses):
        """one damped step through the Schur path -> (d_camera (16,), d_views (V, 6)); nothing is applied"""
        c, vp = _f64(camera, (NCAM,)), _f64(view_poses, (self.V, 6))
        dc, dv = np.zeros(NCAM, np.float64), np.zeros((self.V, 6), np.float64)
        check(self.L.agt_camcal_step(self.h, float(lam), _addr(c), _addr(vp), _addr(dc), _addr(dv)), "agt_camcal_step")
        return dc, dv

    def default_options(self):
        o = Options()
        check(self.L.agt_camcal_default_options(C.byref(o)), "agt_camcal_default_options")
        return o

    def solve(self, camera, view_poses, **options):
        """Levenberg-Marquardt from the given camera and poses -> (camera (16,), view_poses (V, 6), Report); options: fields of Options"""
        c, vp = _f64(camera, (NCAM,)).copy(), _f64(view_poses, (self.V, 6)).copy()
        o = self.default_options()
        for k, v in options.items():
            if v is not None:
                if not hasattr(o, k):
                    raise TypeError("unknown option %r" % k)
                setattr(o, k, v)
        rep = Report()
        check(self.L.agt_camcal_solve(self.h, C.byref(o), _addr(c), _addr(vp), C.byref(rep)), "agt_camcal_solve")
        return c, vp, rep
