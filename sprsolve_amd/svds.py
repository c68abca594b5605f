"""Truncated SVD by thick-restart Lanczos bidiagonalisation, for operators of any shape (no reference analogue)."""
import ctypes as C

import numpy as np

from . import _lib, gen
from .device import DevVec, dev_len, dev_ptr, is_device_array, pre_sync, sfx
from .error import BreakDown, IncompatibleMatrixFormat, InsufficientIterNum, check

WHICH = {"largest": _lib.SVDS_LARGEST, "smallest": _lib.SVDS_SMALLEST}


class Svds:
    """`Svds.new(A, ncv=0, adjoint=None)`: the k largest or smallest singular triplets A v = s u, A^H u = s v of an A of any shape by
    thick-restart Lanczos bidiagonalisation with full reorthogonalisation of both bases; ncv is the basis size,
    3 <= ncv <= min(64, rows, cols), 0 means min(32, rows, cols).  `adjoint` is a handle of A^H (`A.adjoint()`); None lets the
    solver build and own one.  The recurrence is stated in include/sprsolve_hip.h (sprs_svds_*) and runs in C++ on
    device-resident vectors and scalars (sprsolve_amd/csrc/svds.hip, svds_fuse.hpp); the handle holds 2 ncv + 3 work vectors.
    Single GPU."""
    NAME = "svds"

    def __init__(self, A, ncv=0, adjoint=None):
        ncv = int(ncv)
        if ncv < 0:
            raise ValueError("ncv must be >= 0")
        self.A, self.AH = A, adjoint    # borrowed
        self.shape = tuple(A.shape)
        self.dtype = A.dtype
        self.s = sfx(self.dtype)
        self.h = None
        h = C.c_void_p()
        st = getattr(_lib.lib(), "sprs_svds_create_" + self.s)(A.h, adjoint.h if adjoint is not None else None, ncv, C.byref(h))
        if st == _lib.INVALID_ARGUMENT:     # a distributed A, a wrong adjoint, ncv out of range: the library says which
            raise ValueError("sprsolve_hip: invalid argument: " + (_lib.lib().sprs_last_error(A.ctx.h) or b"").decode(errors="replace"))
        check(st, A.ctx.h)
        self.h = h
        self.ncv = ncv or min(32, min(self.shape))

    @classmethod
    def new(cls, A, ncv=0, adjoint=None):
        return cls(A, ncv, adjoint)

    def default_v0(self):
        """The start vector of `solve(v0=None)`: min(rows, cols) entries."""
        n = min(self.shape)
        v = gen.uniform(gen.SEED, n, stream=92)
        if np.dtype(self.dtype).kind == "c":
            v = v + 1j * gen.uniform(gen.SEED, n, stream=93)
        return v.astype(self.dtype)

    def solve(self, k, which="largest", v0=None, max_restarts=1000, tol=0.0, vectors=True):
        """-> (s, U, V, info): s the k singular values in the order of `which`, U of shape (k, rows) and V of shape (k, cols) with
        the singular vectors of s[c] in row c (both None with vectors=False), info = dict(res, nconv, restarts, matvecs) with res
        the absolute residual estimates.  tol = 0.0 selects 1e-10 (f64 / c64) or 1e-4 (f32 / c32); a triplet counts as converged at
        res <= tol * (the largest singular value seen).  v0: a host array or a device vector of min(rows, cols) entries (a device
        v0 takes the device entry point; the results come back as host arrays either way).  Raises SolverError:
        InsufficientIterNum after max_restarts cycles and BreakDown (a NaN, a zero v0, a rank-deficient operator, an invariant
        subspace of fewer than k dimensions) carry what was computed as .s, .U, .V and .info."""
        L = _lib.lib()
        k = int(k)
        if isinstance(which, str):
            if which not in WHICH:
                raise ValueError("which must be 'largest' or 'smallest'")
            which = WHICH[which]
        if tol == 0.0:
            tol = 1e-4 if self.s in "sc" else 1e-10
        rows, cols = self.shape
        if v0 is None:
            v0 = self.default_v0()
        R = _lib.REAL[self.s]
        rdt = np.float32 if self.s in "sc" else np.float64
        kk = max(k, 1)
        vals = np.zeros(kk, rdt); res = np.zeros(kk, rdt)
        nconv = C.c_size_t(0); restarts = C.c_size_t(0); matvecs = C.c_size_t(0)
        pr = C.POINTER(R)
        tail = (res.ctypes.data_as(pr), C.byref(nconv), C.byref(restarts), C.byref(matvecs))
        want = vectors and k > 0
        if is_device_array(v0):
            pre_sync(v0)
            Ud = DevVec(k * rows, self.dtype, self.A.ctx) if want else None
            Vd = DevVec(k * cols, self.dtype, self.A.ctx) if want else None
            st = getattr(L, "sprs_svds_solve_dev_" + self.s)(self.h, k, int(which), dev_ptr(v0), dev_len(v0), int(max_restarts), float(tol),
                                                            vals.ctypes.data_as(pr), Ud.ptr if want else None, k * rows,
                                                            Vd.ptr if want else None, k * cols, *tail)
            keep = want and st in (_lib.OK, _lib.INSUFFICIENT_ITER)
            U = Ud.to_numpy().reshape(k, rows) if keep else None
            V = Vd.to_numpy().reshape(k, cols) if keep else None
            if want:
                Ud.free(); Vd.free()
        else:
            v0a = np.ascontiguousarray(v0, dtype=self.dtype)
            U = np.zeros((k, rows), self.dtype) if want else None
            V = np.zeros((k, cols), self.dtype) if want else None
            st = getattr(L, "sprs_svds_solve_" + self.s)(self.h, k, int(which), v0a.ctypes.data_as(C.c_void_p), v0a.size, int(max_restarts),
                                                        float(tol), vals.ctypes.data_as(pr),
                                                        U.ctypes.data_as(C.c_void_p) if want else None, k * rows,
                                                        V.ctypes.data_as(C.c_void_p) if want else None, k * cols, *tail)
            if st not in (_lib.OK, _lib.INSUFFICIENT_ITER):
                U = V = None
        info = dict(res=res[:k], nconv=nconv.value, restarts=restarts.value, matvecs=matvecs.value)
        vals = vals[:k]
        if st == _lib.OK:
            return vals, U, V, info
        if st == _lib.INCOMPATIBLE_RHS_SIZE:
            raise IncompatibleMatrixFormat("Input vec dimension doesn't match the matrix size")
        if st == _lib.INCOMPATIBLE_X_SIZE:
            raise IncompatibleMatrixFormat("Input and output vec dimension do not match")
        if st in (_lib.INSUFFICIENT_ITER, _lib.BREAKDOWN):
            e = InsufficientIterNum(restarts.value) if st == _lib.INSUFFICIENT_ITER else BreakDown(restarts.value)
            e.s, e.U, e.V, e.info = vals, U, V, info
            raise e
        check(st, self.A.ctx.h)

    def close(self):
        if self.h:
            _lib.lib().sprs_svds_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
