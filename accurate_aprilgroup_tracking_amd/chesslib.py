"""ctypes binding of the chessboard corner finder (include/agt_chess.h -> libagt_chess.so).
Built by build() of __graft_entry__ and loaded by _sidelib.load under the rules of hiplib: there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import ERR_ALLOC, ERR_ARG, ERR_HIP, ERRORS, OK, vp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagt_chess.so")

VERSION = 100
MIN_SIZE, MAX_SIZE, MAX_BATCH, MAX_CANDIDATES, MAX_NMS, MAX_HALF, MAX_ITERS = 11, 8192, 64, 65536, 8, 11, 64
FLAG_CANDIDATES = 1
VERDICT_OK, VERDICT_BORDER, VERDICT_FLAT, VERDICT_SHIFT = 0, 1, 2, 3
DEFAULTS = dict(min_response=200, rel_pct=10, nms=3, half=5, iters=10, max_shift=3.0, min_det=1.0)
_INTS = ("min_response", "rel_pct", "nms", "half", "iters")
# agt_chess_record, 48 bytes
RECORD_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("det", "<f8"), ("shift", "<f8"), ("xf", "<f4"), ("yf", "<f4"), ("verdict", "u1"),
                         ("reserved", "u1", (7,))])
assert RECORD_DTYPE.itemsize == 48

# every symbol include/agt_chess.h declares
SYMBOLS = ["agt_chess_version", "agt_chess_create", "agt_chess_destroy", "agt_chess_response", "agt_chess_candidates", "agt_chess_refine",
           "agt_chess_corners"]


class ChessError(_sidelib.SideLibError):
    """A call of libagt_chess.so returned a negative code."""
    PREFIX, ERRORS = "CHESS", ERRORS


class Options(C.Structure):
    """agt_chess_options"""
    _fields_ = [("min_response", C.c_int32), ("rel_pct", C.c_int32), ("nms", C.c_int32), ("half", C.c_int32), ("iters", C.c_int32),
                ("reserved0", C.c_int32), ("max_shift", C.c_double), ("min_det", C.c_double)]


assert C.sizeof(Options) == 40


def _declare(L):
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    L.agt_chess_version.restype = C.c_int
    L.agt_chess_create.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.agt_chess_destroy.argtypes = [vp]
    L.agt_chess_response.argtypes = [vp, vp, vp, sz, sz, i32, i32, i32, vp]
    L.agt_chess_candidates.argtypes = [vp, vp, vp, sz, sz, i32, i32, i32, C.POINTER(Options), vp, vp]
    L.agt_chess_refine.argtypes = [vp, vp, vp, sz, sz, i32, i32, i32, C.POINTER(Options), vp, vp, vp]
    L.agt_chess_corners.argtypes = [vp, vp, vp, sz, sz, i32, i32, i32, C.POINTER(Options), vp, vp, vp]


_lib = None


def lib():
    """Load libagt_chess.so (once).  Raises RuntimeError when it is missing."""
    global _lib
    if _lib is None:
        _lib = _sidelib.load(LIB_PATH, _declare)
    return _lib


check = ChessError.check


def options(**kw):
    """the defaults with `kw` over them -> Options; an unknown name, an integer option that no int32 holds or a float option that is
    no number is refused here (the ranges are the library's to check)"""
    o = _sidelib.make_options(DEFAULTS, _INTS, ("max_shift", "min_det"), ChessError, "chessboard", kw)
    return Options(*([int(o[k]) for k in _INTS] + [0, float(o["max_shift"]), float(o["min_det"])]))


class Finder(_sidelib.Handle):
    """One agt_chess handle: the workspace for frames of up to width x height in batches of up to max_batch."""
    DESTROY = "agt_chess_destroy"

    def __init__(self, width, height, max_batch=1, max_candidates=1024):
        self.L = lib()
        self.h = C.c_void_p()
        check(self.L.agt_chess_create(int(width), int(height), int(max_batch), int(max_candidates), C.byref(self.h)), "agt_chess_create")

    @staticmethod
    def _opts(opts):
        return C.byref(opts) if opts is not None else None

    def response(self, stream, frames_ptr, pitch, frame_stride, width, height, B, response_ptr):
        """agt_chess_response on raw device addresses (ints or None); enqueues only"""
        check(self.L.agt_chess_response(self.h, vp(stream), vp(frames_ptr), pitch, frame_stride, width, height, B, vp(response_ptr)),
              "agt_chess_response")

    def candidates(self, stream, frames_ptr, pitch, frame_stride, width, height, B, opts, cands_ptr, counts_ptr):
        check(self.L.agt_chess_candidates(self.h, vp(stream), vp(frames_ptr), pitch, frame_stride, width, height, B, self._opts(opts),
                                          vp(cands_ptr), vp(counts_ptr)), "agt_chess_candidates")

    def refine(self, stream, frames_ptr, pitch, frame_stride, width, height, B, opts, cands_ptr, counts_ptr, records_ptr):
        check(self.L.agt_chess_refine(self.h, vp(stream), vp(frames_ptr), pitch, frame_stride, width, height, B, self._opts(opts),
                                      vp(cands_ptr), vp(counts_ptr), vp(records_ptr)), "agt_chess_refine")

    def corners(self, stream, frames_ptr, pitch, frame_stride, width, height, B, opts, cands_ptr, counts_ptr, records_ptr):
        check(self.L.agt_chess_corners(self.h, vp(stream), vp(frames_ptr), pitch, frame_stride, width, height, B, self._opts(opts),
                                       vp(cands_ptr), vp(counts_ptr), vp(records_ptr)), "agt_chess_corners")
