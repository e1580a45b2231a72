"""What the ctypes bindings of this package's libraries share: the load routine (hiplib and every side library's module), and for the
side libraries the error class and the structures and array helpers that more than one of them needs.

A module keeps LIB_PATH, _lib and lib() of its own -- lib() reads the module's LIB_PATH and _lib when it is called -- and hands load()
a function that declares the argument types.
"""
import ctypes as C
import math
import os

import numpy as np


def load(path, declare):
    """CDLL(path) with declare(L) applied.  Raises RuntimeError when the library is missing: there is NO CPU fallback."""
    if not os.path.exists(path):
        raise RuntimeError(
            "HIP extension %s is missing: build it (python -c 'import __graft_entry__ as g; g.build()'). "
            "There is no CPU fallback." % path)
    # PyTorch-ROCm bundles its own libamdhip64.so.7; load it FIRST so that this library's
    # NEEDED libamdhip64.so.7 resolves to the same runtime instance (two HIP runtimes in one
    # process cannot both own the device).
    import torch  # noqa: F401
    L = C.CDLL(path)
    declare(L)
    return L


class SideLibError(ValueError):
    """A call of a side library returned a negative code.  A subclass sets PREFIX (the header's AGT_<PREFIX>_ERR_*) and ERRORS."""
    PREFIX, ERRORS = "", {}

    def __init__(self, code, where):
        self.code = code
        super().__init__("%s failed: AGT_%s_ERR_%s (%d)" % (where, self.PREFIX, self.ERRORS.get(code, "?"), code))

    @classmethod
    def check(cls, rc, where):
        if rc != 0:
            raise cls(rc, where)


class Handle:
    """A handle of a side library (self.L the library, self.h the handle): destroyed by L.<DESTROY> on close(), at the latest when collected."""
    DESTROY = None

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            getattr(self.L, self.DESTROY)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Options(C.Structure):
    """agt_calib_options = agt_camcal_options"""
    _fields_ = [("max_iters", C.c_int32), ("reserved0", C.c_int32), ("ftol", C.c_double), ("lambda0", C.c_double),
                ("lambda_up", C.c_double), ("lambda_down", C.c_double), ("lambda_max", C.c_double)]


class Report(C.Structure):
    """agt_calib_report = agt_camcal_report"""
    _fields_ = [("iterations", C.c_int32), ("accepted", C.c_int32), ("stop_reason", C.c_int32), ("n_residuals", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_rms_px", C.c_double), ("final_lambda", C.c_double)]


STOP_CONVERGED, STOP_MAX_ITERS, STOP_LAMBDA = 1, 2, 3
STOP_NAMES = {STOP_CONVERGED: "converged", STOP_MAX_ITERS: "iteration cap", STOP_LAMBDA: "damping limit"}


def _f64(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))


def _addr(a):
    return C.c_void_p(a.ctypes.data)


# ---- the image stages (tagcode, quadfit, quadfind, draw, chess): raw device addresses in, a batch of 8-bit frames as the input

# agt_side_math.h's codes, under every library's own prefix; a library with more codes adds them to a copy of ERRORS
OK = 0
ERR_ARG, ERR_ALLOC, ERR_HIP = -1, -2, -5
ERRORS = {ERR_ARG: "ARG", ERR_ALLOC: "ALLOC", ERR_HIP: "HIP"}


def vp(a):
    """a raw device address (an int, or None / 0 for NULL) as a ctypes argument"""
    return C.c_void_p(a) if a else None


def make_options(defaults, ints, floats, error_cls, what, kw):
    """`defaults` with `kw` over them -> dict; an unknown name, an option of `ints` that no int32 holds or one of `floats` that is no
    number is refused here (the ranges are the library's to check)"""
    unknown = sorted(set(kw) - set(defaults))
    if unknown:
        raise TypeError("unknown %s option(s) %s (known: %s)" % (what, ", ".join(unknown), ", ".join(defaults)))
    o = dict(defaults, **kw)
    for k in ints:
        if int(o[k]) != o[k] or not -2 ** 31 <= int(o[k]) < 2 ** 31:
            raise error_cls(ERR_ARG, "option %s = %r" % (k, o[k]))
    for k in floats:
        if math.isnan(float(o[k])):
            raise error_cls(ERR_ARG, "option %s = %r" % (k, o[k]))
    return o


def records_numpy(records, dtype):
    """a u8 tensor [..., dtype.itemsize] of records (or its numpy copy) -> structured array [...] of `dtype` (synchronises)"""
    a = records.cpu().numpy() if hasattr(records, "cpu") else np.asarray(records)
    return np.ascontiguousarray(a).view(dtype).reshape(a.shape[:-1])


GRAY_FRAMES = "frames must be cuda u8 [B, H, W] with unit pixel stride"


def is_gray_frames(frames):
    """what the image stages read (any row and frame stride)"""
    import torch
    return isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.is_cuda and frames.dim() == 3 and frames.stride(2) == 1


def check_frames(frames, min_size, width, height, max_batch, error_cls, what):
    """-> (B, h, w) of frames on a workspace `what` made for [max_batch, height, width]"""
    if not is_gray_frames(frames):
        raise ValueError(GRAY_FRAMES)
    B, h, w = frames.shape
    if not (min_size <= w <= width and min_size <= h <= height and 1 <= B <= max_batch):
        raise error_cls(ERR_ARG, "frames of shape %s on a %s for [%d, %d, %d]" % (tuple(frames.shape), what, max_batch, height, width))
    return B, h, w


def frame_args(frames):
    """the call tail every image stage takes: (the current stream of the frames' device, pointer, pitch, frame_stride, width, height, B)"""
    from .cv_hip import _raw_stream
    B, h, w = frames.shape[:3]
    return (_raw_stream(frames.device.index), frames.data_ptr(), frames.stride(1), frames.stride(0), w, h, B)


class PerDevice:
    """cache(device index) -> factory(*args), made with that device current on first use, once per device"""

    def __init__(self, factory, *args):
        self.factory, self.args, self.made = factory, args, {}

    def __call__(self, device):
        if device not in self.made:
            import torch
            with torch.cuda.device(device):
                self.made[device] = self.factory(*self.args)
        return self.made[device]
