"""ctypes binding of the quad finder (include/agt_quadfind.h -> libagt_quadfind.so).
Built by build() of __graft_entry__ and loaded by _sidelib.load under the rules of hiplib: there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import ERR_ALLOC, ERR_ARG, ERR_HIP, ERRORS, OK, vp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagt_quadfind.so")

VERSION = 100
MIN_SIZE, MAX_SIZE, MAX_BATCH, MAX_COMPONENTS, MAX_QUADS = 8, 8192, 64, 65536, 65536
FLAG_QUADS, FLAG_COMPONENTS = 1, 2
DEFAULTS = dict(min_contrast=40, min_area=24, max_area=2 ** 31 - 1, min_fill_pct=5)
# agt_quadfind_record, 32 bytes
RECORD_DTYPE = np.dtype([("label", "<i4"), ("area", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("s2", "<i8")])
assert RECORD_DTYPE.itemsize == 32

# every symbol include/agt_quadfind.h declares
SYMBOLS = ["agt_quadfind_version", "agt_quadfind_create", "agt_quadfind_destroy", "agt_quadfind_detect", "agt_quadfind_labels"]


class QuadFindError(_sidelib.SideLibError):
    """A call of libagt_quadfind.so returned a negative code."""
    PREFIX, ERRORS = "QUADFIND", ERRORS


class Options(C.Structure):
    """agt_quadfind_options"""
    _fields_ = [("min_contrast", C.c_int32), ("min_area", C.c_int32), ("max_area", C.c_int32), ("min_fill_pct", C.c_int32)]


def _declare(L):
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    L.agt_quadfind_version.restype = C.c_int
    L.agt_quadfind_create.argtypes = [i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.agt_quadfind_destroy.argtypes = [vp]
    L.agt_quadfind_detect.argtypes = [vp, vp, vp, sz, sz, i32, i32, i32, C.POINTER(Options), vp, vp, vp]
    L.agt_quadfind_labels.argtypes = [vp, vp, vp, sz, sz, i32, i32, i32, i32, vp]


_lib = None


def lib():
    """Load libagt_quadfind.so (once).  Raises RuntimeError when it is missing."""
    global _lib
    if _lib is None:
        _lib = _sidelib.load(LIB_PATH, _declare)
    return _lib


check = QuadFindError.check


def options(**kw):
    """the defaults with `kw` over them -> Options; an unknown name or a value that no int32 holds is refused here"""
    o = _sidelib.make_options(DEFAULTS, tuple(DEFAULTS), (), QuadFindError, "quad finder", kw)
    return Options(*[int(o[k]) for k in ("min_contrast", "min_area", "max_area", "min_fill_pct")])


class Finder(_sidelib.Handle):
    """One agt_quadfind handle: the workspace for frames of up to width x height in batches of up to max_batch."""
    DESTROY = "agt_quadfind_destroy"

    def __init__(self, width, height, max_batch=1, max_components=4096, max_quads=512):
        self.L = lib()
        self.h = C.c_void_p()
        check(self.L.agt_quadfind_create(int(width), int(height), int(max_batch), int(max_components), int(max_quads), C.byref(self.h)),
              "agt_quadfind_create")

    def detect(self, stream, frames_ptr, pitch, frame_stride, width, height, B, opts, quads_ptr, records_ptr, counts_ptr):
        """agt_quadfind_detect on raw device addresses (ints or None); opts: Options or None; enqueues only"""
        check(self.L.agt_quadfind_detect(self.h, vp(stream), vp(frames_ptr), pitch, frame_stride, width, height, B,
                                         C.byref(opts) if opts is not None else None, vp(quads_ptr), vp(records_ptr), vp(counts_ptr)),
              "agt_quadfind_detect")

    def labels(self, stream, frames_ptr, pitch, frame_stride, width, height, B, min_contrast, labels_ptr):
        """agt_quadfind_labels on raw device addresses; enqueues only"""
        check(self.L.agt_quadfind_labels(self.h, vp(stream), vp(frames_ptr), pitch, frame_stride, width, height, B, int(min_contrast),
                                         vp(labels_ptr)), "agt_quadfind_labels")
