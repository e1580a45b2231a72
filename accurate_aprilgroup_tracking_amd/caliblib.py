"""ctypes binding of the offline calibration library (include/agt_calib.h -> libagt_calib.so).
Built by build() of __graft_entry__ and loaded by _sidelib.load under the rules of hiplib: there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import (Options, Report, STOP_CONVERGED, STOP_MAX_ITERS, STOP_LAMBDA, STOP_NAMES,  # noqa: F401
                       _f64, _addr)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagt_calib.so")

VERSION = 100
OK = 0
ERR_ARG, ERR_ALLOC, ERR_CAMERA, ERR_HIP, ERR_DISCONNECTED, ERR_TOO_FEW_FRAMES, ERR_SINGULAR = -1, -2, -3, -5, -9, -10, -11
ERRORS = {ERR_ARG: "ARG", ERR_ALLOC: "ALLOC", ERR_CAMERA: "CAMERA", ERR_HIP: "HIP", ERR_DISCONNECTED: "DISCONNECTED",
          ERR_TOO_FEW_FRAMES: "TOO_FEW_FRAMES", ERR_SINGULAR: "SINGULAR"}
MAX_TAGS, MAX_FRAMES = 64, 65536

# every symbol include/agt_calib.h declares
SYMBOLS = ["agt_calib_version", "agt_group_calib_create", "agt_group_calib_destroy", "agt_group_calib_eval", "agt_group_calib_step",
           "agt_group_calib_default_options", "agt_group_calib_solve"]


class Problem(C.Structure):
    _fields_ = [("K", C.c_void_p), ("dist", C.c_void_p), ("ndist", C.c_int32), ("n_tags", C.c_int32), ("tag_sizes", C.c_void_p),
                ("anchor", C.c_int32), ("n_frames", C.c_int32), ("n_obs", C.c_int32), ("reserved0", C.c_int32),
                ("obs_frame", C.c_void_p), ("obs_tag", C.c_void_p), ("obs_corners", C.c_void_p)]


class CalibError(_sidelib.SideLibError):
    """A call of libagt_calib.so returned a negative code."""
    PREFIX, ERRORS = "CALIB", ERRORS


def _declare(L):
    vp, f64 = C.c_void_p, C.c_double
    L.agt_calib_version.restype = C.c_int
    L.agt_group_calib_create.argtypes = [C.POINTER(Problem), vp, C.POINTER(vp)]
    L.agt_group_calib_destroy.argtypes = [vp]
    L.agt_group_calib_eval.argtypes = [vp, vp, vp, vp, C.POINTER(f64)]
    L.agt_group_calib_step.argtypes = [vp, f64, vp, vp, vp, vp]
    L.agt_group_calib_default_options.argtypes = [C.POINTER(Options)]
    L.agt_group_calib_solve.argtypes = [vp, C.POINTER(Options), vp, vp, C.POINTER(Report)]


_lib = None


def lib():
    """Load libagt_calib.so (once).  Raises RuntimeError when it is missing."""
    global _lib
    if _lib is None:
        _lib = _sidelib.load(LIB_PATH, _declare)
    return _lib


check = CalibError.check


class GroupCalib(_sidelib.Handle):
    """One agt_group_calib handle: a problem checked, sorted and uploaded once.

    tag_sizes (T,), anchor: tag index, n_frames: F, obs_frame / obs_tag (n,), obs_corners (n, 4, 2); poses are (., 6) rvec | tvec."""
    DESTROY = "agt_group_calib_destroy"

    def __init__(self, cameraMatrix, distCoeffs, tag_sizes, anchor, n_frames, obs_frame, obs_tag, obs_corners, stream=None):
        self.L = lib()
        K = _f64(cameraMatrix, (3, 3))
        dist = None if distCoeffs is None else _f64(distCoeffs, (-1,))
        sizes = _f64(tag_sizes, (-1,))
        fr = np.ascontiguousarray(np.asarray(obs_frame, np.int32).reshape(-1))
        tg = np.ascontiguousarray(np.asarray(obs_tag, np.int32).reshape(-1))
        co = _f64(obs_corners, (-1, 8))
        if not (fr.size == tg.size == co.shape[0]):
            raise ValueError("observation table: %d frames, %d tags, %d corner rows" % (fr.size, tg.size, co.shape[0]))
        self.T, self.F, self.n = int(sizes.size), int(n_frames), int(fr.size)
        p = Problem(_addr(K), None if dist is None or dist.size == 0 else _addr(dist), 0 if dist is None else int(dist.size),
                    self.T, _addr(sizes), int(anchor), self.F, self.n, 0, _addr(fr), _addr(tg), _addr(co))
        self.h = C.c_void_p()
        check(self.L.agt_group_calib_create(C.byref(p), C.c_void_p(stream) if stream else None, C.byref(self.h)), "agt_group_calib_create")

    def eval(self, tag_poses, frame_poses):
        """-> (residuals (n, 8) in the caller's observation order, cost)"""
        tp, fp = _f64(tag_poses, (self.T, 6)), _f64(frame_poses, (self.F, 6))
        res = np.zeros((self.n, 8), np.float64)
        cost = C.c_double()
        check(self.L.agt_group_calib_eval(self.h, _addr(tp), _addr(fp), _addr(res), C.byref(cost)), "agt_group_calib_eval")
        return res, cost.value

    def step(self, lam, tag_poses, frame_poses):
        """one damped step through the Schur path -> (d_tags (T, 6), d_frames (F, 6)); nothing is applied"""
        tp, fp = _f64(tag_poses, (self.T, 6)), _f64(frame_poses, (self.F, 6))
        dt, df = np.zeros((self.T, 6), np.float64), np.zeros((self.F, 6), np.float64)
        check(self.L.agt_group_calib_step(self.h, float(lam), _addr(tp), _addr(fp), _addr(dt), _addr(df)), "agt_group_calib_step")
        return dt, df

    def default_options(self):
        o = Options()
        check(self.L.agt_group_calib_default_options(C.byref(o)), "agt_group_calib_default_options")
        return o

    def solve(self, tag_poses, frame_poses, **options):
        """Levenberg-Marquardt from the given poses -> (tag_poses (T, 6), frame_poses (F, 6), Report); options: fields of Options"""
        tp, fp = _f64(tag_poses, (self.T, 6)).copy(), _f64(frame_poses, (self.F, 6)).copy()
        o = self.default_options()
        for k, v in options.items():
            if v is not None:
                if not hasattr(o, k):
                    raise TypeError("unknown option %r" % k)
                setattr(o, k, v)
        rep = Report()
        check(self.L.agt_group_calib_solve(self.h, C.byref(o), _addr(tp), _addr(fp), C.byref(rep)), "agt_group_calib_solve")
        return tp, fp, rep
