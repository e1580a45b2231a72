"""ctypes binding of the quad edge refinement (include/agt_quadfit.h -> libagt_quadfit.so).

Same rules as tagcodelib: the library is built by `make -C accurate_aprilgroup_tracking_amd/csrc` (build() of __graft_entry__),
there is NO CPU fallback -- a missing library raises --, and torch is imported first so that one HIP runtime owns the device.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagt_quadfit.so")

VERSION = 100
OK = 0
ERR_ARG, ERR_HIP = -1, -5
ERRORS = {ERR_ARG: "ARG", ERR_HIP: "HIP"}
MAX_SIZE, MAX_QUADS, MAX_COORD, MIN_EDGE, MAX_RANGE, MAX_ITERS = 16384, 1 << 20, 1048576.0, 8.0, 16.0, 8
QUAD_OK, QUAD_MASKED, QUAD_DEGENERATE, QUAD_SHORT, QUAD_WEAK, QUAD_DIVERGED = range(6)
STATUS_NAMES = ["OK", "MASKED", "DEGENERATE", "SHORT", "WEAK", "DIVERGED"]
# agt_quad_record, 32 bytes
RECORD_DTYPE = np.dtype([("status", "<i4"), ("passes", "<i4"), ("strength", "<f8"), ("shift", "<f8"), ("resid", "<f8")])
assert RECORD_DTYPE.itemsize == 32

# every symbol include/agt_quadfit.h declares
SYMBOLS = ["agt_quadfit_version", "agt_quad_refine"]


class QuadFitError(ValueError):
    """A call of libagt_quadfit.so returned a negative code."""

    def __init__(self, code, where):
        self.code = code
        super().__init__("%s failed: AGT_QUADFIT_ERR_%s (%d)" % (where, ERRORS.get(code, "?"), code))


_lib = None


def lib():
    """Load libagt_quadfit.so (once).  Raises RuntimeError when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "HIP extension %s is missing: build it (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback." % LIB_PATH)
    import torch  # noqa: F401  (its libamdhip64 first: one HIP runtime per process, see hiplib.lib)
    L = C.CDLL(LIB_PATH)
    vp, i32, sz, f64 = C.c_void_p, C.c_int, C.c_size_t, C.c_double
    L.agt_quadfit_version.restype = C.c_int
    L.agt_quad_refine.argtypes = [vp, vp, sz, sz, i32, i32, i32, vp, vp, i32, f64, i32, f64, vp, vp, vp, vp, vp]
    _lib = L
    return L


def check(rc, where):
    if rc != OK:
        raise QuadFitError(rc, where)


def refine(stream, frames_ptr, pitch, frame_stride, width, height, B, quads_ptr, mask_ptr, Q, range_px, iters, min_strength,
           quads_out_ptr, quads64_out_ptr, records_ptr, ok_ptr, corner_mask_ptr):
    """agt_quad_refine on raw device addresses (ints or None); enqueues only"""
    vp = lambda a: C.c_void_p(a) if a else None
    check(lib().agt_quad_refine(vp(stream), vp(frames_ptr), pitch, frame_stride, width, height, B, vp(quads_ptr), vp(mask_ptr), Q,
                                float(range_px), int(iters), float(min_strength), vp(quads_out_ptr), vp(quads64_out_ptr), vp(records_ptr),
                                vp(ok_ptr), vp(corner_mask_ptr)), "agt_quad_refine")
