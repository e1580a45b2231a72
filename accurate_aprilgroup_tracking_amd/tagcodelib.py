"""ctypes binding of the tag payload decoder (include/agt_tagcode.h -> libagt_tagcode.so).
Built by build() of __graft_entry__ and loaded by _sidelib.load under the rules of hiplib: there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import ERR_ALLOC, ERR_ARG, ERR_HIP, OK, vp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagt_tagcode.so")

VERSION = 100
ERR_FAMILY = -13
ERRORS = {**_sidelib.ERRORS, ERR_FAMILY: "FAMILY"}
MAX_CODES, MAX_SIZE, MAX_QUADS, MAX_COORD = 16384, 16384, 1 << 20, 1048576.0
TAG_OK, TAG_MASKED, TAG_DEGENERATE, TAG_OUTSIDE, TAG_INVERTED, TAG_NO_MATCH, TAG_LOW_MARGIN = range(7)
STATUS_NAMES = ["OK", "MASKED", "DEGENERATE", "OUTSIDE", "INVERTED", "NO_MATCH", "LOW_MARGIN"]
# agt_tag_record, 40 bytes
RECORD_DTYPE = np.dtype([("id", "<i4"), ("hamming", "<i4"), ("rot", "<i4"), ("status", "<i4"), ("margin", "<f8"), ("contrast", "<f8"),
                         ("word", "<u8")])
assert RECORD_DTYPE.itemsize == 40

# every symbol include/agt_tagcode.h declares
SYMBOLS = ["agt_tagcode_version", "agt_tag_family_create", "agt_tag_family_destroy", "agt_tag_decode"]


class TagCodeError(_sidelib.SideLibError):
    """A call of libagt_tagcode.so returned a negative code."""
    PREFIX, ERRORS = "TAGCODE", ERRORS


def _declare(L):
    vp, i32, sz = C.c_void_p, C.c_int, C.c_size_t
    L.agt_tagcode_version.restype = C.c_int
    L.agt_tag_family_create.argtypes = [vp, i32, i32, vp, C.POINTER(vp)]
    L.agt_tag_family_destroy.argtypes = [vp]
    L.agt_tag_decode.argtypes = [vp, vp, sz, sz, i32, i32, i32, vp, vp, i32, vp, i32, C.c_double, vp, vp, vp, vp]


_lib = None


def lib():
    """Load libagt_tagcode.so (once).  Raises RuntimeError when it is missing."""
    global _lib
    if _lib is None:
        _lib = _sidelib.load(LIB_PATH, _declare)
    return _lib


check = TagCodeError.check


class Family(_sidelib.Handle):
    """One agt_tag_family handle: the codes' four rotations, uploaded once; decodes are enqueued on `stream`."""
    DESTROY = "agt_tag_family_destroy"

    def __init__(self, codes, bits_per_side=6, stream=None):
        self.L = lib()
        codes = np.ascontiguousarray(np.asarray(codes, np.uint64).reshape(-1))
        self.n = codes.size
        self.h = C.c_void_p()
        check(self.L.agt_tag_family_create(C.c_void_p(codes.ctypes.data), self.n, int(bits_per_side), vp(stream), C.byref(self.h)), "agt_tag_family_create")

    def decode(self, frames_ptr, pitch, frame_stride, width, height, B, quads_ptr, mask_ptr, Q, expected_ptr, max_hamming, min_margin,
               records_ptr, ok_ptr, corner_mask_ptr, homography_ptr):
        """agt_tag_decode on raw device addresses (ints or None); enqueues only"""
        check(self.L.agt_tag_decode(self.h, vp(frames_ptr), pitch, frame_stride, width, height, B, vp(quads_ptr), vp(mask_ptr), Q,
                                    vp(expected_ptr), int(max_hamming), float(min_margin), vp(records_ptr), vp(ok_ptr), vp(corner_mask_ptr),
                                    vp(homography_ptr)), "agt_tag_decode")
