"""On-chip batch solvers: many small systems with one pattern, one workgroup each (no reference analogue;
include/sprsolve_hip.h, sprs_batch_*)."""
import ctypes as C

import numpy as np

from . import _lib
from .device import NP_OF, default_ctx, dev_len, dev_ptr, dev_sfx, is_device_array, pre_sync, sfx
from .error import DimensionMismatch, ZeorDiagonalElem, check, solve_result

_SOLVERS = {"bicgstab": _lib.BATCH_BICGSTAB, "cg": _lib.BATCH_CG}
_DTYPE_CODE = {"d": 0, "z": 1, "s": 2, "c": 3}
_ARG_ERRORS = (_lib.INCOMPATIBLE_RHS_SIZE, _lib.INCOMPATIBLE_X_SIZE, _lib.DIM_MISMATCH)


class BatchCsr:
    """`BatchCsr.new(n, indptr, indices, values)`: nbatch square systems of n rows that share one CSR pattern (int32 indices, every
    row's columns strictly ascending) and have their own values, a C-contiguous (nbatch, nnz) block.  Vectors are (nbatch, n)
    blocks.  `bicgstab` and `cg` solve all systems in ONE launch: a workgroup runs a whole solve with every vector in the CU's LDS
    (csrc/batch.hip), each system on its own scalars, stopping on its own event.  The recurrences are `BiCGStab`'s and `CG`'s;
    `precond="jacobi"` is the diagonal of each system.  Limits: one pattern per batch; n up to `BatchCsr.max_rows(solver, dtype)`;
    one system per workgroup (systems far below 64 rows waste lanes); Jacobi only; no mixed precision; single GPU."""

    last_status = None   # what the last solve returned: 0, or the status of the lowest-numbered system that did not return 0

    def __init__(self, handle, ctx, dtype, n, nnz, nbatch):
        self.h, self.ctx, self.dtype = handle, ctx, np.dtype(dtype)
        self.n, self.nnz, self.nbatch = int(n), int(nnz), int(nbatch)
        self.s = sfx(self.dtype)

    @classmethod
    def new(cls, n, indptr, indices, values, ctx=None):
        """Host arrays, or device arrays (values a `DevVec` or a torch CUDA tensor of nbatch * nnz scalars; the pattern then as torch
        CUDA int32 tensors, or as host arrays that are uploaded here).  Both are copied: the handle owns its arrays.  Raises ValueError
        with the library's text for a malformed pattern (the lowest row whose columns do not ascend strictly is named)."""
        L = _lib.lib()
        n = int(n)
        dev = is_device_array(values)
        keep = []
        if dev:
            s = dev_sfx(values)
            ctx = ctx or getattr(values, "ctx", None) or default_ctx()
            pat = []
            for a in (indptr, indices):
                if is_device_array(a):
                    if "int32" not in str(a.dtype):
                        raise TypeError("a device pattern must be int32")
                    pat.append(a)
                else:
                    h = np.ascontiguousarray(a, dtype=np.int32)
                    p = C.c_void_p()
                    check(L.sprs_malloc(ctx.h, max(h.nbytes, 4), C.byref(p)), ctx.h)
                    keep.append(p)
                    check(L.sprs_memcpy_h2d(ctx.h, p, h.ctypes.data_as(C.c_void_p), h.nbytes), ctx.h)
                    pat.append((p, h.size))
            plen = [a[1] if isinstance(a, tuple) else dev_len(a) for a in pat]
            pptr = [a[0] if isinstance(a, tuple) else dev_ptr(a) for a in pat]
            pre_sync(indptr, indices, values)
            nnz = plen[1]
            if plen[0] != n + 1:
                raise ValueError("sprsolve_hip: invalid argument: indptr must have n + 1 entries")
            nbatch = dev_len(values) // nnz if nnz else 0
            if dev_len(values) != nbatch * nnz:
                raise ValueError("sprsolve_hip: invalid argument: values must hold nbatch * nnz scalars")
            args = (pptr[0], pptr[1], dev_ptr(values))
            fn = getattr(L, "sprs_batch_create_dev_" + s)
        else:
            ctx = ctx or default_ctx()
            v = np.asarray(values)
            s = sfx(v.dtype)
            rp = np.ascontiguousarray(indptr, dtype=np.int32)
            ci = np.ascontiguousarray(indices, dtype=np.int32)
            nnz = ci.size
            if rp.size != n + 1:
                raise ValueError("sprsolve_hip: invalid argument: indptr must have n + 1 entries")
            if v.ndim != 2 or v.shape[1] != nnz:
                raise ValueError("sprsolve_hip: invalid argument: values must be an (nbatch, nnz) block")
            v = np.ascontiguousarray(v)
            nbatch = v.shape[0]
            keep += [rp, ci, v]
            args = (rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p))
            fn = getattr(L, "sprs_batch_create_" + s)
        h = C.c_void_p(); row = C.c_int64(-1)
        try:
            st = fn(ctx.h, n, int(nnz), int(nbatch), *args, C.byref(h), C.byref(row))
        finally:
            for p in keep:
                if isinstance(p, C.c_void_p):
                    L.sprs_free(ctx.h, p)
        if st == _lib.INVALID_ARGUMENT:
            raise _invalid_argument(ctx)
        check(st, ctx.h)
        return cls(h, ctx, NP_OF[s], n, nnz, nbatch)

    @staticmethod
    def max_rows(solver, dtype):
        """The most rows `solver` ("bicgstab" or "cg") takes for a scalar type."""
        return int(_lib.lib().sprs_batch_max_rows(_SOLVERS[solver], _DTYPE_CODE[sfx(dtype)]))

    @property
    def info(self):
        """dict(n, nnz, nbatch, threads, lds_cg, lds_bicgstab): the threads of a workgroup and the LDS bytes it asks for."""
        v = [C.c_int64() for _ in range(6)]
        check(_lib.lib().sprs_batch_info(self.h, *[C.byref(x) for x in v]), self.ctx.h)
        return dict(zip(("n", "nnz", "nbatch", "threads", "lds_cg", "lds_bicgstab"), (x.value for x in v)))

    def set_values(self, values):
        """Replaces the values of all systems (an (nbatch, nnz) block on the host, or nbatch * nnz scalars on the device); the
        pattern and the plan stay."""
        L = _lib.lib()
        if is_device_array(values):
            if dev_sfx(values) != self.s or dev_len(values) != self.nbatch * self.nnz:
                raise ValueError("sprsolve_hip: invalid argument: values must hold nbatch * nnz scalars of %s" % self.dtype)
            pre_sync(values)
            st = getattr(L, "sprs_batch_set_values_dev_" + self.s)(self.h, dev_ptr(values))
        else:
            v = np.ascontiguousarray(values, dtype=self.dtype)
            if v.shape != (self.nbatch, self.nnz):
                raise ValueError("sprsolve_hip: invalid argument: values must be an (nbatch, nnz) block")
            st = getattr(L, "sprs_batch_set_values_" + self.s)(self.h, v.ctypes.data_as(C.c_void_p))
        check(st, self.ctx.h)

    def values(self):
        """The (nbatch, nnz) block of values, read back."""
        v = np.zeros((self.nbatch, self.nnz), self.dtype)
        check(getattr(_lib.lib(), "sprs_batch_read_" + self.s)(self.h, v.ctypes.data_as(C.c_void_p)), self.ctx.h)
        return v

    def _blocks(self, a, b, what):
        """-> (is device, pointer a, length a, pointer b, length b, keep) of an input block and an in/out block."""
        dev = is_device_array(a)
        if dev != is_device_array(b):
            raise TypeError("%s must both be host arrays or both be device vectors" % what)
        if dev:
            pre_sync(a, b)
            return True, dev_ptr(a), dev_len(a), dev_ptr(b), dev_len(b), None
        a_h = np.ascontiguousarray(a, dtype=self.dtype)
        if not (isinstance(b, np.ndarray) and b.dtype == self.dtype and b.flags.c_contiguous):
            raise TypeError("the output block must be a C-contiguous %s ndarray (it is written in place)" % self.dtype)
        return False, a_h.ctypes.data_as(C.c_void_p), a_h.size, b.ctypes.data_as(C.c_void_p), b.size, a_h

    def mul_vec(self, X, Y):
        """Y_b = A_b X_b for every system, in one launch; (nbatch, n) blocks on the host, or device vectors."""
        dev, xp, xl, yp, yl, _keep = self._blocks(X, Y, "X and Y")
        st = getattr(_lib.lib(), "sprs_batch_mul_vec%s_%s" % ("_dev" if dev else "", self.s))(self.h, xp, xl, yp, yl)
        if st == _lib.DIM_MISMATCH:
            raise DimensionMismatch("Dimension mismatch")
        check(st, self.ctx.h)

    def _solve(self, name, rhs, x, max_iter, tol, precond):
        if precond not in (None, "jacobi"):
            raise ValueError("sprsolve_hip: invalid argument: precond must be None or 'jacobi'")
        dev, rp, rl, xp, xl, _keep = self._blocks(rhs, x, "rhs and x")
        R = _lib.REAL[self.s]
        n_out = max(self.nbatch, 1)
        its = (C.c_size_t * n_out)(); res = (R * n_out)(); status = (C.c_int * n_out)()
        st = getattr(_lib.lib(), "sprs_batch_%s_solve%s_%s" % (name, "_dev" if dev else "", self.s))(
            self.h, _lib.BATCH_JACOBI if precond else _lib.BATCH_NONE, rp, rl, xp, xl, int(max_iter), float(tol), its, res, status)
        self.last_status = int(st)
        if st == _lib.INVALID_ARGUMENT:
            raise _invalid_argument(self.ctx)
        if st == _lib.ZERO_DIAGONAL:
            raise ZeorDiagonalElem(int(its[0]))
        if st >= _lib.ERR_HIP or st in _ARG_ERRORS:
            solve_result(st, 0, 0.0, self.ctx.h)
        nb = self.nbatch
        return (np.array(its[:nb], dtype=np.int64), np.array(res[:nb], dtype=np.dtype(R)), np.array(status[:nb], dtype=np.int32))

    def bicgstab(self, rhs, x, max_iter, tol, precond=None):
        """-> (its, res, status): arrays of nbatch entries, what `BiCGStab.solve` / `.precond_solve` reports per system and the
        system's status code (0 = Ok, 3 InsufficientIterNum, 4 BreakDown).  Solver events are reported, never raised; argument
        errors raise.  x is in/out.  precond: None or "jacobi" (ZeorDiagonalElem where the pattern lacks a diagonal entry)."""
        return self._solve("bicgstab", rhs, x, max_iter, tol, precond)

    def cg(self, rhs, x, max_iter, tol, precond=None):
        """The same with `CG`'s recurrence, for Hermitian positive-definite systems (status 5 = InvalidPreconditioner with
        "jacobi", res = re(conj(r).M^-1 r))."""
        return self._solve("cg", rhs, x, max_iter, tol, precond)

    def close(self):
        if self.h:
            _lib.lib().sprs_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _invalid_argument(ctx):
    return ValueError("sprsolve_hip: invalid argument: " + (_lib.lib().sprs_last_error(ctx.h) or b"").decode(errors="replace"))
