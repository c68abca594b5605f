"""Preconditioned block eigensolver (LOBPCG) for Hermitian operators (no reference analogue)."""
import numpy as np

from . import _lib
from ._solver import _Handle, applied_prefix, eig_call, eig_result, in_vec, stream_vector, which_and_tol
from .device import DevVec, is_device_array
from .eigsh import WHICH
from .precond import DiagPrecond


class Lobpcg(_Handle):
    """`Lobpcg.new(A, size, block=0)`: the k <= block algebraically smallest or largest eigenpairs of a Hermitian A (not checked,
    as with CG) by locally optimal block preconditioned conjugate gradients; block is the number of vectors iterated,
    1 <= block <= 8 and 6 block <= n, 0 means min(8, n // 6).  The recurrence is stated in include/sprsolve_hip.h
    (sprs_lobpcg_*) and runs in C++ on device-resident vectors and scalars (sprsolve_amd/csrc/lobpcg.hip, lobpcg_fuse.hpp); the
    handle holds 6 block work vectors.  Single GPU."""
    NAME = "lobpcg"
    SAYS_WHY = True     # a distributed A, block out of range

    def __init__(self, A, size, block=0):
        block = int(block)
        if block < 0:
            raise ValueError("block must be >= 0")
        self.size = int(size)
        self._create(A, self.size, block)
        self.block = block or min(_lib.LOBPCG_MAX_BLOCK, self.size // 6)

    @classmethod
    def new(cls, A, size, block=0):
        return cls(A, size, block)

    def default_X0(self):
        """The start block of `solve(X0=None)`, shape (block, n): what the library generates for a null X0."""
        return np.stack([stream_vector(self.size, self.dtype, 100 + 2 * c) for c in range(self.block)])

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
        k = int(k)
        which, tol = which_and_tol(which, tol, self.s, WHICH)
        prefix = applied_prefix(precond)
        if precond is not None and (prefix in (None, "bjacobi")) and not isinstance(precond, DiagPrecond):    # (no sprs_bjacobi_lobpcg_*)
            raise TypeError("precond must be a DiagPrecond, ILU0, AMG or FSAI")
        own = None
        if X0 is not None and not is_device_array(X0) and prefix is not None:     # an applied handle has the device entry only
            X0 = own = DevVec.from_numpy(np.ascontiguousarray(X0, dtype=self.dtype).reshape(-1), self.A.ctx)
        try:
            x0p, x0l, dev, _keep = in_vec(X0, self.dtype)
            st, vals, (X,), res, (nconv, iters, restarts, matvecs) = eig_call(
                self, "lobpcg" if prefix is None else prefix + "_lobpcg", dev or prefix is not None,
                (precond.h if precond is not None else None, k, which, x0p, x0l, int(max_iter), tol), k, (self.size,), vectors and k > 0, 4)
        finally:
            if own is not None:
                own.free()
        info = dict(res=res, nconv=nconv, iters=iters, restarts=restarts, matvecs=matvecs)
        return eig_result(st, (vals, X, info), ("vals", "X", "info"), iters, self.A.ctx.h,
                          "Input block dimension doesn't match block * matrix size")
