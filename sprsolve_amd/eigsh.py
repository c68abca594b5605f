"""Thick-restart Lanczos eigensolver for Hermitian operators (no reference analogue)."""
import ctypes as C

import numpy as np

from . import _lib, gen
from .device import DevVec, dev_len, dev_ptr, is_device_array, pre_sync, sfx
from .error import BreakDown, IncompatibleMatrixFormat, InsufficientIterNum, check

WHICH = {"largest": _lib.EIGSH_LARGEST, "smallest": _lib.EIGSH_SMALLEST}


class Eigsh:
    """`Eigsh.new(A, size, ncv=0)`: the k algebraically largest or smallest eigenpairs of a Hermitian A (not checked, as with
    CG) by thick-restart Lanczos with full reorthogonalisation; ncv is the basis size, 3 <= ncv <= min(64, n), 0 means
    min(32, n).  The recurrence is stated in include/sprsolve_hip.h (sprs_eigsh_*) and runs in C++ on device-resident vectors
    and scalars (sprsolve_amd/csrc/eigsh.hip, eigsh_fuse.hpp); the handle holds ncv + 2 work vectors.  Single GPU."""
    NAME = "eigsh"

    def __init__(self, A, size, ncv=0):
        ncv = int(ncv)
        if ncv < 0:
            raise ValueError("ncv must be >= 0")
        self.A = A                      # borrowed
        self.size = int(size)
        self.dtype = A.dtype
        self.s = sfx(self.dtype)
        self.h = None
        h = C.c_void_p()
        st = getattr(_lib.lib(), "sprs_eigsh_create_" + self.s)(A.h, self.size, ncv, C.byref(h))
        if st == _lib.INVALID_ARGUMENT:     # a distributed A, ncv out of range: the library says which
            raise ValueError("sprsolve_hip: invalid argument: " + (_lib.lib().sprs_last_error(A.ctx.h) or b"").decode(errors="replace"))
        check(st, A.ctx.h)
        self.h = h
        self.ncv = ncv or min(32, self.size)

    @classmethod
    def new(cls, A, size, ncv=0):
        return cls(A, size, ncv)

    def default_v0(self):
        """The start vector of `solve(v0=None)`."""
        v = gen.uniform(gen.SEED, self.size, stream=90)
        if np.dtype(self.dtype).kind == "c":
            v = v + 1j * gen.uniform(gen.SEED, self.size, stream=91)
        return v.astype(self.dtype)

    def solve(self, k, which="largest", v0=None, max_restarts=1000, tol=0.0, vectors=True):
        """-> (vals, X, info): vals the k Ritz values in the order of `which`, X of shape (k, n) with eigenvector c in row c (None
        with vectors=False), info = dict(res, nconv, restarts, matvecs) with res the absolute residual estimates.  tol = 0.0
        selects 1e-10 (f64 / c64) or 1e-4 (f32 / c32); a pair counts as converged at res <= tol * (the largest |Ritz value| seen).
        v0: a host array or a device vector of n entries (a device v0 takes the device entry point; the results come back as
        host arrays either way).  Raises SolverError: InsufficientIterNum after max_restarts cycles and BreakDown (a NaN, a zero
        v0, an invariant subspace of fewer than k dimensions) carry what was computed as .vals, .X and .info."""
        L = _lib.lib()
        k = int(k)
        if isinstance(which, str):
            if which not in WHICH:
                raise ValueError("which must be 'largest' or 'smallest'")
            which = WHICH[which]
        if tol == 0.0:
            tol = 1e-4 if self.s in "sc" else 1e-10
        n = self.size
        if v0 is None:
            v0 = self.default_v0()
        R = _lib.REAL[self.s]
        rdt = np.float32 if self.s in "sc" else np.float64
        kk = max(k, 1)
        vals = np.zeros(kk, rdt); res = np.zeros(kk, rdt)
        nconv = C.c_size_t(0); restarts = C.c_size_t(0); matvecs = C.c_size_t(0)
        pr = C.POINTER(R)
        tail = (res.ctypes.data_as(pr), C.byref(nconv), C.byref(restarts), C.byref(matvecs))
        if is_device_array(v0):
            pre_sync(v0)
            Xd = DevVec(k * n, self.dtype, self.A.ctx) if vectors and k > 0 else None
            st = getattr(L, "sprs_eigsh_solve_dev_" + self.s)(self.h, k, int(which), dev_ptr(v0), dev_len(v0), int(max_restarts), float(tol),
                                                             vals.ctypes.data_as(pr), Xd.ptr if Xd is not None else None, k * n, *tail)
            X = Xd.to_numpy().reshape(k, n) if Xd is not None and st in (_lib.OK, _lib.INSUFFICIENT_ITER) else None
            if Xd is not None:
                Xd.free()
        else:
            v0a = np.ascontiguousarray(v0, dtype=self.dtype)
            X = np.zeros((k, n), self.dtype) if vectors and k > 0 else None
            st = getattr(L, "sprs_eigsh_solve_" + self.s)(self.h, k, int(which), v0a.ctypes.data_as(C.c_void_p), v0a.size, int(max_restarts),
                                                         float(tol), vals.ctypes.data_as(pr),
                                                         X.ctypes.data_as(C.c_void_p) if X is not None else None, k * n, *tail)
            if st not in (_lib.OK, _lib.INSUFFICIENT_ITER):
                X = None
        info = dict(res=res[:k], nconv=nconv.value, restarts=restarts.value, matvecs=matvecs.value)
        vals = vals[:k]
        if st == _lib.OK:
            return vals, X, info
        if st == _lib.INCOMPATIBLE_RHS_SIZE:
            raise IncompatibleMatrixFormat("Input vec dimension doesn't match the matrix size")
        if st == _lib.INCOMPATIBLE_X_SIZE:
            raise IncompatibleMatrixFormat("Input and output vec dimension do not match")
        if st in (_lib.INSUFFICIENT_ITER, _lib.BREAKDOWN):
            e = InsufficientIterNum(restarts.value) if st == _lib.INSUFFICIENT_ITER else BreakDown(restarts.value)
            e.vals, e.X, e.info = vals, X, info
            raise e
        check(st, self.A.ctx.h)

    def close(self):
        if self.h:
            _lib.lib().sprs_eigsh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
