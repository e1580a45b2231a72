"""ctypes binding of the quad edge refinement (include/agt_quadfit.h -> libagt_quadfit.so).
Built by build() of __graft_entry__ and loaded by _sidelib.load under the rules of hiplib: there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import ERR_ARG, ERR_HIP, ERRORS, OK, vp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagt_quadfit.so")

VERSION = 100
MAX_SIZE, MAX_QUADS, MAX_COORD, MIN_EDGE, MAX_RANGE, MAX_ITERS = 16384, 1 << 20, 1048576.0, 8.0, 16.0, 8
QUAD_OK, QUAD_MASKED, QUAD_DEGENERATE, QUAD_SHORT, QUAD_WEAK, QUAD_DIVERGED = range(6)
STATUS_NAMES = ["OK", "MASKED", "DEGENERATE", "SHORT", "WEAK", "DIVERGED"]
# agt_quad_record, 32 bytes
RECORD_DTYPE = np.dtype([("status", "<i4"), ("passes", "<i4"), ("strength", "<f8"), ("shift", "<f8"), ("resid", "<f8")])
assert RECORD_DTYPE.itemsize == 32

# every symbol include/agt_quadfit.h declares
SYMBOLS = ["agt_quadfit_version", "agt_quad_refine"]


class QuadFitError(_sidelib.SideLibError):
    """A call of libagt_quadfit.so returned a negative code."""
    PREFIX, ERRORS = "QUADFIT", ERRORS


def _declare(L):
    vp, i32, sz, f64 = C.c_void_p, C.c_int, C.c_size_t, C.c_double
    L.agt_quadfit_version.restype = C.c_int
    L.agt_quad_refine.argtypes = [vp, vp, sz, sz, i32, i32, i32, vp, vp, i32, f64, i32, f64, vp, vp, vp, vp, vp]


_lib = None


def lib():
    """Load libagt_quadfit.so (once).  Raises RuntimeError when it is missing."""
    global _lib
    if _lib is None:
        _lib = _sidelib.load(LIB_PATH, _declare)
    return _lib


check = QuadFitError.check


def refine(stream, frames_ptr, pitch, frame_stride, width, height, B, quads_ptr, mask_ptr, Q, range_px, iters, min_strength,
           quads_out_ptr, quads64_out_ptr, records_ptr, ok_ptr, corner_mask_ptr):
    """agt_quad_refine on raw device addresses (ints or None); enqueues only"""
    check(lib().agt_quad_refine(vp(stream), vp(frames_ptr), pitch, frame_stride, width, height, B, vp(quads_ptr), vp(mask_ptr), Q,
                                float(range_px), int(iters), float(min_strength), vp(quads_out_ptr), vp(quads64_out_ptr), vp(records_ptr),
                                vp(ok_ptr), vp(corner_mask_ptr)), "agt_quad_refine")
