"""Factorised sparse approximate inverse (FSAI) preconditioner (no reference analogue; include/sprsolve_hip.h, sprs_fsai_*)."""
import ctypes as C

import numpy as np

from . import _lib
from .device import dev_len, dev_ptr, is_device_array, pre_sync, sfx
from .error import DimensionMismatch, InvalidPreconditioner, ZeorDiagonalElem, check
from .mat import HipCsr, MatVecMul


class FSAI(MatVecMul):
    """`FSAI.new(A, power=1)`: M = G^H G for a square single-GPU `HipCsr` that is Hermitian positive definite, G sparse lower
    triangular on the lower part of the pattern of A (power=1) or of A A (power=2), its rows computed on the device
    (csrc/fsai.hip).  Only the stored entries of A's lower triangle are read.  As a `MatVecMul` it applies M, two ordinary SpMVs
    through the handles `G` and `GH`; `CG`, `GMRES`, `BiCGStab` and `MinRes` take it in `precond_solve` in place of a
    `DiagPrecond`.  The handle owns its factors: A may be closed afterwards."""

    def __init__(self, handle, ctx, dtype, n):
        self.h, self.ctx, self.dtype, self.n = handle, ctx, np.dtype(dtype), int(n)
        self.s = sfx(self.dtype)

    @classmethod
    def new(cls, A, power=1):
        """Raises IncompatibleMatrixFormat (not square), ValueError (power not 1 or 2, distributed A, unsorted or duplicate
        columns, a row of G longer than 64), ZeorDiagonalElem(row) for a missing diagonal entry, or InvalidPreconditioner where
        A is not positive definite on the pattern."""
        if power not in (1, 2):
            raise ValueError("sprsolve_hip: invalid argument: power must be 1 or 2, got %r" % (power,))
        h = C.c_void_p(); row = C.c_int64(-1)
        st = _lib.lib().sprs_fsai_create(A.h, int(power), C.byref(h), C.byref(row))
        if st == _lib.ZERO_DIAGONAL:
            raise ZeorDiagonalElem(row.value)
        if st == _lib.INVALID_PRECOND:
            raise InvalidPreconditioner("A is not positive definite on the pattern at row %d" % row.value)
        if st == _lib.INVALID_ARGUMENT:
            raise ValueError("sprsolve_hip: invalid argument: " + (_lib.lib().sprs_last_error(A.ctx.h) or b"").decode(errors="replace"))
        check(st, A.ctx.h)
        return cls(h, A.ctx, A.dtype, A.rows())

    @property
    def info(self):
        """dict(n, nnz, max_row, power): rows, nnz(G), the longest row of G and the pattern's power."""
        v = [C.c_int64() for _ in range(4)]
        check(_lib.lib().sprs_fsai_info(self.h, *[C.byref(x) for x in v]), self.ctx.h)
        return dict(zip(("n", "nnz", "max_row", "power"), (x.value for x in v)))

    def _view(self, which):
        h = C.c_void_p()
        check(_lib.lib().sprs_fsai_factor(self.h, which, C.byref(h)), self.ctx.h)
        return _FactorView(h, self.ctx, self.dtype, (self.n, self.n), keepalive=self)

    @property
    def G(self):
        """G as a non-owning `HipCsr` view (valid while this handle lives)."""
        return self._view(0)

    @property
    def GH(self):
        """G^H = `sprs_csr_adjoint(G, 1)` as a non-owning `HipCsr` view."""
        return self._view(1)

    def factor(self):
        """(indptr, indices, data) of G."""
        return self.G.to_host()

    def _apply(self, v_in, v_out, checked=True):
        L = _lib.lib()
        if is_device_array(v_in):
            if checked and (self.n != dev_len(v_in) or self.n != dev_len(v_out)):
                raise DimensionMismatch("Dimension mismatch")
            pre_sync(v_in, v_out)
            check(getattr(L, "sprs_fsai_mul_vec_dev_" + self.s)(self.h, dev_ptr(v_in), dev_ptr(v_out)), self.ctx.h)
            self.ctx.sync()
            return
        x = np.ascontiguousarray(v_in, dtype=self.dtype)
        if not (isinstance(v_out, np.ndarray) and v_out.dtype == self.dtype and v_out.flags.c_contiguous):
            raise TypeError("v_out must be a contiguous %s ndarray" % self.dtype)
        check(getattr(L, "sprs_fsai_mul_vec_" + self.s)(self.h, x.ctypes.data_as(C.c_void_p), x.size,
                                                        v_out.ctypes.data_as(C.c_void_p), v_out.size), self.ctx.h)

    def mul_vec(self, v_in, v_out):
        """v_out = G^H (G v_in); host arrays or device vectors (v_in may be v_out)."""
        self._apply(v_in, v_out)

    def mul_vec_unchecked(self, v_in, v_out):
        self._apply(v_in, v_out, checked=False)

    def mul_vec_dot(self, v_in, v_out):
        raise NotImplementedError("a preconditioner has no fused dot product (as DiagPrecond)")

    def mul_vec_dot_unchecked(self, v_in, v_out):
        raise NotImplementedError("a preconditioner has no fused dot product (as DiagPrecond)")

    def close(self):
        if self.h:
            _lib.lib().sprs_fsai_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _FactorView(HipCsr):
    """A factor of an `FSAI`: the handle belongs to the preconditioner and is never destroyed through the view."""

    def close(self):
        self.h = None
