"""Thick-restart Lanczos eigensolver for Hermitian operators (no reference analogue)."""
from . import _lib
from ._solver import _Handle, eig_call, eig_result, in_vec, stream_vector, which_and_tol

WHICH = {"largest": _lib.EIGSH_LARGEST, "smallest": _lib.EIGSH_SMALLEST}


class Eigsh(_Handle):
    """`Eigsh.new(A, size, ncv=0)`: the k algebraically largest or smallest eigenpairs of a Hermitian A (not checked, as with
    CG) by thick-restart Lanczos with full reorthogonalisation; ncv is the basis size, 3 <= ncv <= min(64, n), 0 means
    min(32, n).  The recurrence is stated in include/sprsolve_hip.h (sprs_eigsh_*) and runs in C++ on device-resident vectors
    and scalars (sprsolve_amd/csrc/eigsh.hip, eigsh_fuse.hpp); the handle holds ncv + 2 work vectors.  Single GPU."""
    NAME = "eigsh"
    SAYS_WHY = True     # a distributed A, ncv out of range

    def __init__(self, A, size, ncv=0):
        ncv = int(ncv)
        if ncv < 0:
            raise ValueError("ncv must be >= 0")
        self.size = int(size)
        self._create(A, self.size, ncv)
        self.ncv = ncv or min(32, self.size)

    @classmethod
    def new(cls, A, size, ncv=0):
        return cls(A, size, ncv)

    def default_v0(self):
        """The start vector of `solve(v0=None)`."""
        return stream_vector(self.size, self.dtype, 90)

    def solve(self, k, which="largest", v0=None, max_restarts=1000, tol=0.0, vectors=True):
        """-> (vals, X, info): vals the k Ritz values in the order of `which`, X of shape (k, n) with eigenvector c in row c (None
        with vectors=False), info = dict(res, nconv, restarts, matvecs) with res the absolute residual estimates.  tol = 0.0
        selects 1e-10 (f64 / c64) or 1e-4 (f32 / c32); a pair counts as converged at res <= tol * (the largest |Ritz value| seen).
        v0: a host array or a device vector of n entries (a device v0 takes the device entry point; the results come back as
        host arrays either way).  Raises SolverError: InsufficientIterNum after max_restarts cycles and BreakDown (a NaN, a zero
        v0, an invariant subspace of fewer than k dimensions) carry what was computed as .vals, .X and .info."""
        k = int(k)
        which, tol = which_and_tol(which, tol, self.s, WHICH)
        v0p, v0l, dev, _keep = in_vec(self.default_v0() if v0 is None else v0, self.dtype)
        st, vals, (X,), res, (nconv, restarts, matvecs) = eig_call(
            self, "eigsh", dev, (k, which, v0p, v0l, int(max_restarts), tol), k, (self.size,), vectors and k > 0, 3)
        info = dict(res=res, nconv=nconv, restarts=restarts, matvecs=matvecs)
        return eig_result(st, (vals, X, info), ("vals", "X", "info"), restarts, self.A.ctx.h)
