"""What the ctypes bindings of this package's libraries share: the load routine (hiplib and every side library's module), and for the
side libraries the error class and the structures and array helpers that more than one of them needs.

A module keeps LIB_PATH, _lib and lib() of its own -- lib() reads the module's LIB_PATH and _lib when it is called -- and hands load()
a function that declares the argument types.
"""
import ctypes as C
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
