"""LSMR least squares for operators of any shape (no reference analogue)."""
import ctypes as C

import numpy as np

from . import _lib
from ._solver import _SolverBase
from .device import dev_len, dev_ptr, is_device_array, pre_sync
from .error import solve_result


class LSMR(_SolverBase):
    """`LSMR.new(A, adjoint=None)`: min |rhs - A x|_2 (damped: |[A; damp I] x - [rhs; 0]|_2) for A of any shape.  `adjoint` is a
    handle of A^H (`A.adjoint()`); None lets the solver build and own one.  The recurrence is stated in include/sprsolve_hip.h
    (sprs_lsmr_*) and runs in C++ on device-resident vectors and scalars (sprsolve_amd/csrc/lsmr.hip, lsmr_fuse.hpp)."""
    KIND = _lib.SOLVER_LSMR
    NAME = "lsmr"

    def __init__(self, A, adjoint=None):
        self.AH = adjoint                       # borrowed
        self.size = A.shape
        self._create(A, adjoint.h if adjoint is not None else None)

    @classmethod
    def new(cls, A, adjoint=None):
        return cls(A, adjoint)

    def solve(self, rhs, x, max_iter, tol, damp=0.0):
        """x (cols entries) is in/out: a non-zero x is the initial guess.  Returns (iters, |r| / |rhs|, |A^H r| / (|A| |r|)) as the
        recurrence estimates them; raises SolverError (BreakDown on a non-finite norm), DimensionMismatch, ValueError (damp < 0)."""
        L = _lib.lib()
        its = C.c_size_t(0); res = _lib.REAL[self.s](0.0); ares = _lib.REAL[self.s](0.0)
        dev = is_device_array(rhs)
        if dev != is_device_array(x):
            raise TypeError("rhs and x must both be host arrays or both be device vectors")
        if dev:
            pre_sync(rhs, x)
            st = getattr(L, "sprs_lsmr_solve_dev_" + self.s)(self.h, dev_ptr(rhs), dev_len(rhs), dev_ptr(x), dev_len(x), float(damp),
                                                            int(max_iter), float(tol), C.byref(its), C.byref(res), C.byref(ares))
        else:
            rhs_a = np.ascontiguousarray(rhs, dtype=self.dtype)
            if not (isinstance(x, np.ndarray) and x.dtype == self.dtype and x.flags.c_contiguous):
                raise TypeError("x must be a contiguous %s ndarray (it is updated in place)" % self.dtype)
            st = getattr(L, "sprs_lsmr_solve_" + self.s)(self.h, rhs_a.ctypes.data_as(C.c_void_p), rhs_a.size, x.ctypes.data_as(C.c_void_p),
                                                        x.size, float(damp), int(max_iter), float(tol), C.byref(its), C.byref(res),
                                                        C.byref(ares))
        if st == _lib.OK:
            return its.value, res.value, ares.value
        return solve_result(st, its.value, res.value, self.A.ctx.h)
