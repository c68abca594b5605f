"""Conjugate gradients on several right-hand sides at once (no reference analogue)."""
import ctypes as C

import numpy as np

from . import _lib
from ._solver import _Handle, column_call
from .device import dev_len, dev_ptr, is_device_array, pre_sync


class CGMany(_Handle):
    """`CGMany.new(A, size, k)`: CG (see `CG`) on up to k <= 8 right-hand sides in three launches per iteration whatever k is
    (sprsolve_amd/csrc/spmm.hip, cg_many_fuse.hpp, cg_many.hip).  A block of right-hand sides is a C-contiguous (size, k) array.
    Every column runs the recurrence of include/sprsolve_hip.h (sprs_cg_*) on its own scalars and stops on its own event."""

    NAME = "cgmany"
    last_status = None  # what the last solve returned: 0, or the status of the lowest-numbered column that did not return 0

    def __init__(self, A, size, k):
        self.size, self.k = int(size), int(k)
        if self.k < 0:
            raise ValueError("sprsolve_hip: invalid argument")
        self._create(A, self.size, self.k)

    @classmethod
    def new(cls, A, size, k):
        return cls(A, size, k)

    def solve(self, rhs, x, max_iter, tol):
        """-> (its, res, status): arrays of k entries, what CG.solve reports per column and the column's status code (0 = Ok,
        3 InsufficientIterNum, 4 BreakDown).  Solver events are reported, never raised; argument errors raise.  x is in/out."""
        return self._solve(None, rhs, x, max_iter, tol)

    def precond_solve(self, precond, rhs, x, max_iter, tol):
        """Jacobi-preconditioned (status 5 = InvalidPreconditioner, res = re(conj(r).M^-1 r))."""
        if precond is None:
            raise ValueError("sprsolve_hip: invalid argument")
        return self._solve(precond, rhs, x, max_iter, tol)

    def _solve(self, precond, rhs, x, max_iter, tol):
        L = _lib.lib()
        dev = is_device_array(rhs)
        if dev != is_device_array(x):
            raise TypeError("rhs and x must both be host arrays or both be device vectors")
        ph = precond.h if precond is not None else None
        if dev:
            pre_sync(rhs, x)
            rl, xl = dev_len(rhs), dev_len(x)
            k = rl // self.size if self.size else 0
            fn, rp, xp = getattr(L, "sprs_cgmany_solve_dev_" + self.s), dev_ptr(rhs), dev_ptr(x)
        else:
            rhs_a = np.asarray(rhs)
            if rhs_a.ndim != 2 or not isinstance(x, np.ndarray) or x.ndim != 2:
                raise TypeError("rhs and x must be 2-D (size, k) blocks")
            rhs_a = np.ascontiguousarray(rhs_a, dtype=self.dtype)
            if not (x.dtype == self.dtype and x.flags.c_contiguous):
                raise TypeError("x must be a C-contiguous %s ndarray (it is updated in place)" % self.dtype)
            k, rl, xl = rhs_a.shape[1], rhs_a.size, x.size
            if x.shape[1] != k:
                from .error import IncompatibleMatrixFormat
                raise IncompatibleMatrixFormat("Input and output vec dimension do not match")
            fn, rp, xp = getattr(L, "sprs_cgmany_solve_" + self.s), rhs_a.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p)
        return column_call(self, int(k), lambda its, res, status: fn(self.h, ph, rp, rl, xp, xl, int(k), int(max_iter), float(tol), its, res, status))
