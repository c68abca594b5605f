"""ILU(0) preconditioner with level-scheduled or Jacobi-sweep triangular solves (no reference analogue; include/sprsolve_hip.h,
sprs_ilu0_*)."""
import ctypes as C

import numpy as np

from . import _lib
from .device import dev_len, dev_ptr, is_device_array, pre_sync, sfx
from .error import DimensionMismatch, ZeorDiagonalElem, check
from .mat import MatVecMul


class ILU0(MatVecMul):
    """`ILU0.new(A)`: the incomplete LU factorisation of a square single-GPU `HipCsr` on A's own pattern.  As a `MatVecMul` it
    applies M^-1 = U^-1 L^-1 (two triangular solves, level by level: csrc/ilu0.hip); `CG.precond_solve` and
    `GMRES.precond_solve` take it in place of a `DiagPrecond`.  The handle owns its factors: A may be closed afterwards.
    `ILU0.new(A, sweeps=k)`, k >= 1: the same factors, each triangular solve replaced by k Jacobi sweeps from zero (the header's
    statement): one fully parallel launch per sweep instead of one per dependency level, 2k - 2 launches per application.  With
    k at least the level count the sweeps return the exact solves bit for bit; a handful is usually enough for a preconditioner.
    `ILU0.new(A, order="multicolor")` or `order=perm` (int32, new -> old): the factorisation of P A P^T, applied as
    P^T U^-1 L^-1 P on vectors in A's numbering; under the multicolour ordering a solve has at most as many levels as colours."""

    def __init__(self, handle, ctx, dtype, n, nnz):
        self.h, self.ctx, self.dtype, self.n, self.nnz = handle, ctx, np.dtype(dtype), int(n), int(nnz)
        self.s = sfx(self.dtype)

    @classmethod
    def new(cls, A, sweeps=0, order=None):
        """sweeps = 0: exact level-scheduled solves; 1 .. 4096: that many Jacobi sweeps per triangular solve.
        order = None: A's own row order; "multicolor": rows sorted by `A.color(0)`; an int32 permutation (new -> old): that one.
        Raises IncompatibleMatrixFormat (not square), ValueError (distributed A, unsorted or duplicate columns, a sweep count
        outside 0 .. 4096, a bad permutation, an ordering together with sweeps) or ZeorDiagonalElem(row), row in A's numbering:
        a missing diagonal entry, or a pivot that is exactly zero or not finite."""
        sweeps = int(sweeps)
        if not 0 <= sweeps <= 4096:
            raise ValueError("sprsolve_hip: invalid argument: sweeps must be in 0 .. 4096 (0 = exact solves), got %d" % sweeps)
        h = C.c_void_p(); row = C.c_int64(-1)
        if order is None:
            st = _lib.lib().sprs_ilu0_create_sweeps(A.h, sweeps, C.byref(h), C.byref(row))
        elif isinstance(order, str):
            if order != "multicolor":
                raise ValueError("sprsolve_hip: invalid argument: order must be None, \"multicolor\" or a permutation, got %r" % order)
            st = _lib.lib().sprs_ilu0_create_ordered(A.h, sweeps, _lib.ORDER_MULTICOLOR, None, 0, C.byref(h), C.byref(row))
        else:
            perm = np.ascontiguousarray(order, dtype=np.int32)
            st = _lib.lib().sprs_ilu0_create_ordered(A.h, sweeps, _lib.ORDER_PERM, perm.ctypes.data_as(C.c_void_p), perm.size, C.byref(h), C.byref(row))
        if st == _lib.ZERO_DIAGONAL:
            raise ZeorDiagonalElem(row.value)
        if st == _lib.INVALID_ARGUMENT:
            raise ValueError("sprsolve_hip: invalid argument: " + (_lib.lib().sprs_last_error(A.ctx.h) or b"").decode(errors="replace"))
        check(st, A.ctx.h)
        return cls(h, A.ctx, A.dtype, A.rows(), A.nnz())

    @property
    def sweeps(self):
        """Jacobi sweeps per triangular solve; 0 for exact solves."""
        return int(_lib.lib().sprs_ilu0_sweeps(self.h))

    @property
    def order(self):
        """The permutation (int32, new -> old) of an ordered handle, None for one in A's own order."""
        if _lib.lib().sprs_ilu0_order(self.h, None) != 1:
            return None
        perm = np.empty(self.n, np.int32)
        _lib.lib().sprs_ilu0_order(self.h, perm.ctypes.data_as(C.c_void_p))
        return perm

    @property
    def levels(self):
        """dict(lower_levels, upper_levels, lower_launches, upper_launches): dependency levels of the two solves and the kernel
        launches one application of each costs (a sweeps handle: sweeps - 1 and sweeps)."""
        v = [C.c_int64() for _ in range(4)]
        check(_lib.lib().sprs_ilu0_levels(self.h, *[C.byref(x) for x in v]), self.ctx.h)
        return dict(zip(("lower_levels", "upper_levels", "lower_launches", "upper_launches"), (x.value for x in v)))

    def factors(self):
        """The nnz factor values at A's CSR positions: l_ik below the diagonal, u_ij on and above it."""
        out = np.zeros(self.nnz, self.dtype)
        check(_lib.lib().sprs_ilu0_read(self.h, out.ctypes.data_as(C.c_void_p)), self.ctx.h)
        return out

    def _apply(self, which, v_in, v_out, checked=True):
        L = _lib.lib()
        if is_device_array(v_in):
            if checked and (self.n != dev_len(v_in) or self.n != dev_len(v_out)):
                raise DimensionMismatch("Dimension mismatch")
            pre_sync(v_in, v_out)
            check(getattr(L, "sprs_ilu0_solve_dev_" + self.s)(self.h, which, dev_ptr(v_in), dev_ptr(v_out)), self.ctx.h)
            self.ctx.sync()
            return
        x = np.ascontiguousarray(v_in, dtype=self.dtype)
        if not (isinstance(v_out, np.ndarray) and v_out.dtype == self.dtype and v_out.flags.c_contiguous):
            raise TypeError("v_out must be a contiguous %s ndarray" % self.dtype)
        check(getattr(L, "sprs_ilu0_solve_" + self.s)(self.h, which, x.ctypes.data_as(C.c_void_p), x.size,
                                                      v_out.ctypes.data_as(C.c_void_p), v_out.size), self.ctx.h)

    def mul_vec(self, v_in, v_out):
        """v_out = U^-1 (L^-1 v_in), exactly or by sweeps as the handle was created; host arrays or device vectors (v_in may be v_out)."""
        self._apply(0, v_in, v_out)

    def mul_vec_unchecked(self, v_in, v_out):
        self._apply(0, v_in, v_out, checked=False)

    def solve_lower(self, v_in, v_out):
        """v_out = L^-1 v_in (L unit lower)."""
        self._apply(1, v_in, v_out)

    def solve_upper(self, v_in, v_out):
        """v_out = U^-1 v_in."""
        self._apply(2, v_in, v_out)

    def mul_vec_dot(self, v_in, v_out):
        raise NotImplementedError("a preconditioner has no fused dot product (as DiagPrecond)")

    def mul_vec_dot_unchecked(self, v_in, v_out):
        raise NotImplementedError("a preconditioner has no fused dot product (as DiagPrecond)")

    def close(self):
        if self.h:
            _lib.lib().sprs_ilu0_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
