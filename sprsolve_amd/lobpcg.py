"""Preconditioned block eigensolver (LOBPCG) for Hermitian operators (no reference analogue)."""
import ctypes as C

import numpy as np

from . import _lib, gen
from .amg import AMG
from .device import DevVec, dev_len, dev_ptr, is_device_array, pre_sync, sfx
from .eigsh import WHICH
from .error import BreakDown, IncompatibleMatrixFormat, InsufficientIterNum, check
from .fsai import FSAI
from .ilu import ILU0
from .precond import DiagPrecond

_APPLIED = ((ILU0, "ilu0"), (AMG, "amg"), (FSAI, "fsai"))


class Lobpcg:
    """`Lobpcg.new(A, size, block=0)`: the k <= block algebraically smallest or largest eigenpairs of a Hermitian A (not checked,
    as with CG) by locally optimal block preconditioned conjugate gradients; block is the number of vectors iterated,
    1 <= block <= 8 and 6 block <= n, 0 means min(8, n // 6).  The recurrence is stated in include/sprsolve_hip.h
    (sprs_lobpcg_*) and runs in C++ on device-resident vectors and scalars (sprsolve_amd/csrc/lobpcg.hip, lobpcg_fuse.hpp); the
    handle holds 6 block work vectors.  Single GPU."""
    NAME = "lobpcg"

    def __init__(self, A, size, block=0):
        block = int(block)
        if block < 0:
            raise ValueError("block must be >= 0")
        self.A = A                      # borrowed
        self.size = int(size)
        self.dtype = A.dtype
        self.s = sfx(self.dtype)
        self.h = None
        h = C.c_void_p()
        st = getattr(_lib.lib(), "sprs_lobpcg_create_" + self.s)(A.h, self.size, block, C.byref(h))
        if st == _lib.INVALID_ARGUMENT:     # a distributed A, block out of range: the library says which
            raise ValueError("sprsolve_hip: invalid argument: " + (_lib.lib().sprs_last_error(A.ctx.h) or b"").decode(errors="replace"))
        check(st, A.ctx.h)
        self.h = h
        self.block = block or min(_lib.LOBPCG_MAX_BLOCK, self.size // 6)

    @classmethod
    def new(cls, A, size, block=0):
        return cls(A, size, block)

    def default_X0(self):
        """The start block of `solve(X0=None)`, shape (block, n): what the library generates for a null X0."""
        X = np.zeros((self.block, self.size), self.dtype)
        for c in range(self.block):
            v = gen.uniform(gen.SEED, self.size, stream=100 + 2 * c)
            if np.dtype(self.dtype).kind == "c":
                v = v + 1j * gen.uniform(gen.SEED, self.size, stream=101 + 2 * c)
            X[c] = v.astype(self.dtype)
        return X

    def solve(self, k, which="smallest", precond=None, X0=None, max_iter=1000, tol=0.0, vectors=True):
        """-> (vals, X, info): vals the first k Ritz values in the order of `which`, X of shape (k, n) with eigenvector c in row c
        (None with vectors=False), info = dict(res, nconv, iters, restarts, matvecs) with res the absolute residual norms and
        restarts the count of [X, W] fallbacks.  precond: None, a `DiagPrecond`, `ILU0`, `AMG` or `FSAI`.  tol = 0.0 selects
        1e-10 (f64 / c64) or 1e-4 (f32 / c32); a pair counts as converged at res <= tol * anorm, anorm the largest |Rayleigh
        quotient| of an X or W column seen (at most |A|_2), and is soft-locked while it stays there.
        X0: a host array of shape (block, n) or a device vector of block * n entries, vector after vector (a device X0 takes
        the device entry point; the results come back as host arrays either way); None: `default_X0()`.  Raises SolverError:
        InsufficientIterNum after max_iter iterations and BreakDown (a NaN, a zero or dependent column of X0) carry what was
        computed as .vals, .X and .info."""
        L = _lib.lib()
        k = int(k)
        if isinstance(which, str):
            if which not in WHICH:
                raise ValueError("which must be 'largest' or 'smallest'")
            which = WHICH[which]
        if tol == 0.0:
            tol = 1e-4 if self.s in "sc" else 1e-10
        n = self.size
        prefix = None
        for cls, name in _APPLIED:
            if isinstance(precond, cls):
                prefix = name
        if precond is not None and prefix is None and not isinstance(precond, DiagPrecond):
            raise TypeError("precond must be a DiagPrecond, ILU0, AMG or FSAI")
        R = _lib.REAL[self.s]
        rdt = np.float32 if self.s in "sc" else np.float64
        kk = max(k, 1)
        vals = np.zeros(kk, rdt); res = np.zeros(kk, rdt)
        cnt = [C.c_size_t(0) for _ in range(4)]
        pr = C.POINTER(R)
        tail = (res.ctypes.data_as(pr),) + tuple(C.byref(c) for c in cnt)
        ph = precond.h if precond is not None else None
        ok = (_lib.OK, _lib.INSUFFICIENT_ITER)
        own = None
        if X0 is not None and not is_device_array(X0) and prefix is not None:     # an applied handle has the device entry only
            X0 = own = DevVec.from_numpy(np.ascontiguousarray(X0, dtype=self.dtype).reshape(-1), self.A.ctx)
        try:
            if prefix is not None or is_device_array(X0):
                if X0 is not None:
                    pre_sync(X0)
                Xd = DevVec(k * n, self.dtype, self.A.ctx) if vectors and k > 0 else None
                name = "sprs_lobpcg_solve_dev_" if prefix is None else "sprs_%s_lobpcg_solve_dev_" % prefix
                st = getattr(L, name + self.s)(self.h, ph, k, int(which), dev_ptr(X0) if X0 is not None else None,
                                               dev_len(X0) if X0 is not None else 0, int(max_iter), float(tol), vals.ctypes.data_as(pr),
                                               Xd.ptr if Xd is not None else None, k * n, *tail)
                X = Xd.to_numpy().reshape(k, n) if Xd is not None and st in ok else None
                if Xd is not None:
                    Xd.free()
            else:
                X0a = np.ascontiguousarray(X0, dtype=self.dtype) if X0 is not None else None
                X = np.zeros((k, n), self.dtype) if vectors and k > 0 else None
                st = getattr(L, "sprs_lobpcg_solve_" + self.s)(self.h, ph, k, int(which), X0a.ctypes.data_as(C.c_void_p) if X0a is not None else None,
                                                               X0a.size if X0a is not None else 0, int(max_iter), float(tol), vals.ctypes.data_as(pr),
                                                               X.ctypes.data_as(C.c_void_p) if X is not None else None, k * n, *tail)
                if st not in ok:
                    X = None
        finally:
            if own is not None:
                own.free()
        nconv, iters, restarts, matvecs = (c.value for c in cnt)
        info = dict(res=res[:k], nconv=nconv, iters=iters, restarts=restarts, matvecs=matvecs)
        vals = vals[:k]
        if st == _lib.OK:
            return vals, X, info
        if st == _lib.INCOMPATIBLE_RHS_SIZE:
            raise IncompatibleMatrixFormat("Input block dimension doesn't match block * matrix size")
        if st == _lib.INCOMPATIBLE_X_SIZE:
            raise IncompatibleMatrixFormat("Input and output vec dimension do not match")
        if st in (_lib.INSUFFICIENT_ITER, _lib.BREAKDOWN):
            e = InsufficientIterNum(iters) if st == _lib.INSUFFICIENT_ITER else BreakDown(iters)
            e.vals, e.X, e.info = vals, X, info
            raise e
        check(st, self.A.ctx.h)

    def close(self):
        if self.h:
            _lib.lib().sprs_lobpcg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
