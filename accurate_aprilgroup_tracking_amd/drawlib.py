"""ctypes binding of the drawing stage (include/agt_draw.h -> libagt_draw.so).
Built by build() of __graft_entry__ and loaded by _sidelib.load under the rules of hiplib: there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

from . import _sidelib
from ._sidelib import ERR_ARG, ERR_HIP, ERRORS, OK, vp

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libagt_draw.so")

VERSION = 100
MAX_SIZE_PX, MAX_PRIMS, MAX_TOTAL, MAX_POINTS, MAX_COORD, MAX_SIZE, CHUNK = 16384, 4096, 1 << 20, 4096, 32767, 64, 256
NONE, DISC, SEGMENT = range(3)
CLEAR = 1
F32, F64 = 0, 1
# agt_draw_prim, 32 bytes
PRIM_DTYPE = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("size", "<i4"), ("color", "u1", (4,)),
                       ("reserved", "<i4")])
assert PRIM_DTYPE.itemsize == 32

# every symbol include/agt_draw.h declares
SYMBOLS = ["agt_draw_version", "agt_draw_raster", "agt_draw_pose_lists"]


class DrawError(_sidelib.SideLibError):
    """A call of libagt_draw.so returned a negative code."""
    PREFIX, ERRORS = "DRAW", ERRORS


def _declare(L):
    vp, i32, u32, sz = C.c_void_p, C.c_int, C.c_uint32, C.c_size_t
    L.agt_draw_version.restype = C.c_int
    L.agt_draw_raster.argtypes = [vp, vp, sz, sz, i32, i32, i32, i32, vp, i32, C.c_uint]
    L.agt_draw_pose_lists.argtypes = [vp, vp, i32, i32, i32, vp, sz, i32, i32, i32, i32, i32, u32, u32, vp, vp]


_lib = None


def lib():
    """Load libagt_draw.so (once).  Raises RuntimeError when it is missing."""
    global _lib
    if _lib is None:
        _lib = _sidelib.load(LIB_PATH, _declare)
    return _lib


check = DrawError.check


def pack_color(color):
    """(B, G, R) or one gray level -> B | G << 8 | R << 16, the colour argument of agt_draw_pose_lists"""
    c = [int(v) for v in np.ravel(color)]
    c = (c * 3 if len(c) == 1 else c)[:3]
    if len(c) != 3 or any(v < 0 or v > 255 for v in c):
        raise ValueError("a colour is one level or (B, G, R), each 0..255")
    return c[0] | (c[1] << 8) | (c[2] << 16)


def prims(records):
    """[(kind, x0, y0, x1, y1, size, (B, G, R)), ...] -> PRIM_DTYPE array (a host-side display list)"""
    out = np.zeros(len(records), PRIM_DTYPE)
    for o, (kind, x0, y0, x1, y1, size, color) in zip(out, records):
        o["kind"], o["x0"], o["y0"], o["x1"], o["y1"], o["size"] = kind, x0, y0, x1, y1, size
        o["color"][:3] = color
    return out


def raster(stream, frames_ptr, pitch, frame_stride, width, height, channels, B, prims_ptr, P, flags=0):
    """agt_draw_raster on raw device addresses (ints or None); enqueues only"""
    check(lib().agt_draw_raster(vp(stream), vp(frames_ptr), pitch, frame_stride, width, height, channels, B, vp(prims_ptr), P, flags),
          "agt_draw_raster")


def pose_lists(stream, points_ptr, dtype, n, B, gate_ptr, gate_stride, width, height, corners_per_tag, radius, thickness, dot_color,
               line_color, dots_ptr, outline_ptr):
    """agt_draw_pose_lists on raw device addresses (ints or None); enqueues only"""
    check(lib().agt_draw_pose_lists(vp(stream), vp(points_ptr), dtype, n, B, vp(gate_ptr), gate_stride, width, height, corners_per_tag,
                                    radius, thickness, dot_color, line_color, vp(dots_ptr), vp(outline_ptr)), "agt_draw_pose_lists")
