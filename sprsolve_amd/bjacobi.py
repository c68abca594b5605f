"""Block-Jacobi preconditioner (no reference analogue; include/sprsolve_hip.h, sprs_bjacobi_*)."""
import ctypes as C

import numpy as np

from . import _lib
from .device import dev_len, dev_ptr, is_device_array, pre_sync, sfx
from .error import DimensionMismatch, InvalidPreconditioner, check
from .mat import MatVecMul


class BlockJacobi(MatVecMul):
    """`BlockJacobi.new(A, block_size=bs)` or `BlockJacobi.new(A, block_ptr=[0, .., n])`: M = blockdiag(A_bb)^-1 for a square
    single-GPU `HipCsr`, the diagonal blocks of at most 32 rows (the unknowns of one grid node, or one grid line) inverted on the
    device by Gauss-Jordan elimination with row pivoting (csrc/bjacobi.hip).  As a `MatVecMul` it applies M in one launch;
    `CG`, `GMRES`, `BiCGStab` and `MinRes` take it in place of a `DiagPrecond` (MINRES with the real types only: see the header);
    `IDRS` and `Lobpcg` do not take it yet (TypeError).  The handle owns its blocks: A may be closed afterwards."""

    def __init__(self, handle, ctx, dtype, n):
        self.h, self.ctx, self.dtype, self.n = handle, ctx, np.dtype(dtype), int(n)
        self.s = sfx(self.dtype)

    @classmethod
    def new(cls, A, block_size=None, block_ptr=None):
        """Raises IncompatibleMatrixFormat (not square), ValueError (both or neither of block_size and block_ptr, a block_ptr that
        does not run from 0 to n strictly increasing, a block of more than 32 rows, distributed A, unsorted or duplicate columns) or
        InvalidPreconditioner naming the rows of the first singular block."""
        h = C.c_void_p(); row = C.c_int64(-1)
        bs = 0 if block_size is None else int(block_size)
        if block_size is not None and bs <= 0:
            raise ValueError("sprsolve_hip: invalid argument: block_size must be positive, got %r" % (block_size,))
        bp = None if block_ptr is None else np.ascontiguousarray(block_ptr, dtype=np.int64)
        if bp is not None and (bp.ndim != 1 or bp.size < 1):
            raise ValueError("sprsolve_hip: invalid argument: block_ptr must be a one-dimensional array of nblocks + 1 entries")
        st = _lib.lib().sprs_bjacobi_create(A.h, bs, None if bp is None else bp.ctypes.data_as(C.c_void_p), 0 if bp is None else bp.size - 1,
                                            C.byref(h), C.byref(row))
        if st == _lib.INVALID_PRECOND:
            s = row.value
            e = min(s + bs, A.rows()) if bp is None else int(bp[np.searchsorted(bp, s, side="right")])
            raise InvalidPreconditioner("the diagonal block of rows %d .. %d is singular" % (s, e - 1))
        if st == _lib.INVALID_ARGUMENT:
            raise ValueError("sprsolve_hip: invalid argument: " + (_lib.lib().sprs_last_error(A.ctx.h) or b"").decode(errors="replace"))
        check(st, A.ctx.h)
        return cls(h, A.ctx, A.dtype, A.rows())

    @property
    def info(self):
        """dict(n, nblocks, max_block, slots): rows, blocks, the largest block and the slots of the packed storage."""
        v = [C.c_int64() for _ in range(4)]
        check(_lib.lib().sprs_bjacobi_info(self.h, *[C.byref(x) for x in v]), self.ctx.h)
        return dict(zip(("n", "nblocks", "max_block", "slots"), (x.value for x in v)))

    @property
    def block_ptr(self):
        """The nblocks + 1 block starts."""
        bp = np.zeros(self.info["nblocks"] + 1, np.int64)
        check(_lib.lib().sprs_bjacobi_block_ptr(self.h, bp.ctypes.data_as(C.c_void_p)), self.ctx.h)
        return bp

    def inverse(self):
        """The inverse blocks as a list of (m, m) arrays."""
        bp = self.block_ptr
        m = np.diff(bp)
        flat = np.zeros(int(np.sum(m * m)), self.dtype)
        check(getattr(_lib.lib(), "sprs_bjacobi_inverse_" + self.s)(self.h, flat.ctypes.data_as(C.c_void_p), flat.size), self.ctx.h)
        off = np.concatenate([[0], np.cumsum(m * m)])
        return [flat[off[b]:off[b + 1]].reshape(m[b], m[b]) for b in range(m.size)]

    def _apply(self, v_in, v_out, checked=True):
        L = _lib.lib()
        if is_device_array(v_in):
            if checked and (self.n != dev_len(v_in) or self.n != dev_len(v_out)):
                raise DimensionMismatch("Dimension mismatch")
            pre_sync(v_in, v_out)
            check(getattr(L, "sprs_bjacobi_mul_vec_dev_" + self.s)(self.h, dev_ptr(v_in), dev_ptr(v_out)), self.ctx.h)
            self.ctx.sync()
            return
        x = np.ascontiguousarray(v_in, dtype=self.dtype)
        if not (isinstance(v_out, np.ndarray) and v_out.dtype == self.dtype and v_out.flags.c_contiguous):
            raise TypeError("v_out must be a contiguous %s ndarray" % self.dtype)
        check(getattr(L, "sprs_bjacobi_mul_vec_" + self.s)(self.h, x.ctypes.data_as(C.c_void_p), x.size,
                                                           v_out.ctypes.data_as(C.c_void_p), v_out.size), self.ctx.h)

    def mul_vec(self, v_in, v_out):
        """v_out = blockdiag(A_bb)^-1 v_in; host arrays or device vectors (v_in may be v_out)."""
        self._apply(v_in, v_out)

    def mul_vec_unchecked(self, v_in, v_out):
        self._apply(v_in, v_out, checked=False)

    def mul_vec_dot(self, v_in, v_out):
        raise NotImplementedError("a preconditioner has no fused dot product (as DiagPrecond)")

    def mul_vec_dot_unchecked(self, v_in, v_out):
        raise NotImplementedError("a preconditioner has no fused dot product (as DiagPrecond)")

    def close(self):
        if self.h:
            _lib.lib().sprs_bjacobi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
