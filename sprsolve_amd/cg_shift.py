"""Multi-shift conjugate gradients: (A + sigma_j I) x_j = rhs for several shifts in one Krylov run (no reference analogue)."""
import ctypes as C

import numpy as np

from . import _lib
from ._solver import _Handle, column_call
from .device import dev_len, dev_ptr, is_device_array, pre_sync


class CGShift(_Handle):
    """`CGShift.new(A, size, mmax)`: the solutions of (A + sigma_j I) x_j = rhs for up to mmax <= 8 real shifts sigma_j >= 0 and a
    Hermitian positive-definite A, in one CG run on A: one SpMV and three launches per iteration whatever the number of shifts
    (sprsolve_amd/csrc/cg_shift_fuse.hpp, cg_shift.hip; the recurrence: include/sprsolve_hip.h, sprs_cgshift_*).  The method starts
    from x = 0 and takes no preconditioner.  The solutions are m contiguous vectors: a C-contiguous (m, size) array."""

    NAME = "cgshift"
    SAYS_WHY = True     # a distributed A, mmax out of range; in a solve the number of shifts, a negative or non-finite shift
    last_status = None  # what the last solve returned: 0, or the status of the lowest-numbered column that did not return 0

    def __init__(self, A, size, mmax):
        self.size, self.mmax = int(size), int(mmax)
        if self.mmax < 0:
            raise ValueError("sprsolve_hip: invalid argument")
        self._create(A, self.size, self.mmax)

    @classmethod
    def new(cls, A, size, mmax):
        return cls(A, size, mmax)

    def solve(self, shifts, rhs, x, max_iter, tol):
        """-> (its, res, status): arrays of m = len(shifts) entries, what CG.solve on A + sigma_j I reports per column and the
        column's status code (0 = Ok, 3 InsufficientIterNum, 4 BreakDown).  Solver events are reported, never raised; argument
        errors raise.  rhs: size entries; x: (m, size), output only (a device vector of m * size entries).  Host arrays or
        device vectors, both of one kind."""
        L = _lib.lib()
        R = _lib.REAL[self.s]
        sh = np.ascontiguousarray(np.asarray(shifts, dtype=np.dtype(R)).ravel())
        m = int(sh.size)
        dev = is_device_array(rhs)
        if dev != is_device_array(x):
            raise TypeError("rhs and x must both be host arrays or both be device vectors")
        if dev:
            pre_sync(rhs, x)
            rl, xl = dev_len(rhs), dev_len(x)
            fn, rp, xp = getattr(L, "sprs_cgshift_solve_dev_" + self.s), dev_ptr(rhs), dev_ptr(x)
        else:
            rhs_a = np.ascontiguousarray(np.asarray(rhs), dtype=self.dtype)
            if rhs_a.ndim != 1 or not isinstance(x, np.ndarray) or x.ndim != 2:
                raise TypeError("rhs must be 1-D (size) and x a 2-D (m, size) block")
            if not (x.dtype == self.dtype and x.flags.c_contiguous):
                raise TypeError("x must be a C-contiguous %s ndarray (it is written in place)" % self.dtype)
            rl, xl = rhs_a.size, x.size
            fn, rp, xp = getattr(L, "sprs_cgshift_solve_" + self.s), rhs_a.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p)
        return column_call(self, m, lambda its, res, status: fn(self.h, sh.ctypes.data_as(C.POINTER(R)), m, rp, rl, xp, xl, int(max_iter),
                                                                float(tol), its, res, status))
