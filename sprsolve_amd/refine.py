"""Mixed-precision iterative refinement over the single-precision Krylov solvers (no reference analogue)."""
import ctypes as C

import numpy as np

from . import _lib
from .device import dev_len, dev_ptr, is_device_array, pre_sync, sfx
from .error import check, solve_result
from .mat import HipCsr

_INNER = {"cg": _lib.INNER_CG, "gmres": _lib.INNER_GMRES}
_LOW = {"d": np.float32, "z": np.complex64}


class _BorrowedCsr(HipCsr):
    """A handle owned by someone else (kept alive through `keepalive`): closing the view releases nothing."""

    def close(self):
        self.h = None


class Refine:
    """`Refine.new(A, size, inner="cg", restart=30, precond=None)` for an f64 / c64 operator A: the residual and the solution
    stay in A's precision, every correction is an inner CG or GMRES(restart) solve in f32 / c32 on a copy of A rounded once
    (sprsolve_amd/csrc/refine.hip, refine_fuse.hpp).  The recurrence is stated in include/sprsolve_hip.h (sprs_refine_*).
    `precond` is a Jacobi DiagPrecond of A's scalar type; the inner solves use its single-precision copy.  Single GPU."""

    def __init__(self, A, size, inner="cg", restart=30, precond=None):
        self.A, self.size, self.dtype, self.precond = A, int(size), A.dtype, precond
        self.s = sfx(self.dtype)
        if self.s not in _LOW:
            raise TypeError("Refine takes an f64 / Complex<f64> operator (got %s)" % self.dtype)
        if inner not in _INNER:
            raise ValueError("inner must be 'cg' or 'gmres'")
        if int(restart) < 0:
            raise ValueError("sprsolve_hip: invalid argument")
        L = _lib.lib()
        h = C.c_void_p()
        st = getattr(L, "sprs_refine_create_" + self.s)(A.h, self.size, precond.h if precond is not None else None, _INNER[inner],
                                                        int(restart), C.byref(h))
        if st == _lib.INVALID_ARGUMENT:
            text = (L.sprs_last_error(A.ctx.h) or b"").decode(errors="replace")
            raise ValueError("sprsolve_hip: invalid argument" + (": " + text if text else ""))
        check(st, A.ctx.h)
        self.h = h
        self.low = _BorrowedCsr(C.c_void_p(L.sprs_refine_low_csr(h)), A.ctx, _LOW[self.s], A.shape, keepalive=self)

    @classmethod
    def new(cls, A, size, inner="cg", restart=30, precond=None):
        return cls(A, size, inner, restart, precond)

    def solve(self, rhs, x, max_outer, tol, inner_max_iter, inner_tol):
        """-> (outer, inner_its, res): the outer steps made, the sum of the inner solves' iteration counts, the relative
        residual |rhs - A x| / |rhs| in A's precision.  Raises SolverError: InsufficientIterNum(max_outer), or what an inner
        solve ended in other than Ok / InsufficientIterNum (BreakDown, InvalidPreconditioner).  x is in/out."""
        L = _lib.lib()
        outer = C.c_size_t(0); inner = C.c_size_t(0); res = C.c_double(0.0)
        dev = is_device_array(rhs)
        if dev != is_device_array(x):
            raise TypeError("rhs and x must both be host arrays or both be device vectors")
        if dev:
            pre_sync(rhs, x)
            fn, rp, rl, xp, xl = getattr(L, "sprs_refine_solve_dev_" + self.s), dev_ptr(rhs), dev_len(rhs), dev_ptr(x), dev_len(x)
        else:
            rhs_a = np.ascontiguousarray(rhs, dtype=self.dtype)
            if not (isinstance(x, np.ndarray) and x.dtype == self.dtype and x.flags.c_contiguous):
                raise TypeError("x must be a contiguous %s ndarray (it is updated in place)" % self.dtype)
            fn, rp, rl, xp, xl = (getattr(L, "sprs_refine_solve_" + self.s), rhs_a.ctypes.data_as(C.c_void_p), rhs_a.size,
                                  x.ctypes.data_as(C.c_void_p), x.size)
        st = fn(self.h, rp, rl, xp, xl, int(max_outer), float(tol), int(inner_max_iter), float(inner_tol), C.byref(outer),
                C.byref(inner), C.byref(res))
        self.last = (outer.value, inner.value, res.value)      # also what an error left behind
        solve_result(st, outer.value, res.value, self.A.ctx.h)
        return outer.value, inner.value, res.value

    def close(self):
        if self.h:
            self.low.close()
            _lib.lib().sprs_refine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
