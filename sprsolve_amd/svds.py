"""Truncated SVD by thick-restart Lanczos bidiagonalisation, for operators of any shape (no reference analogue)."""
from . import _lib
from ._solver import _Handle, eig_call, eig_result, in_vec, stream_vector, which_and_tol

WHICH = {"largest": _lib.SVDS_LARGEST, "smallest": _lib.SVDS_SMALLEST}


class Svds(_Handle):
    """`Svds.new(A, ncv=0, adjoint=None)`: the k largest or smallest singular triplets A v = s u, A^H u = s v of an A of any shape by
    thick-restart Lanczos bidiagonalisation with full reorthogonalisation of both bases; ncv is the basis size,
    3 <= ncv <= min(64, rows, cols), 0 means min(32, rows, cols).  `adjoint` is a handle of A^H (`A.adjoint()`); None lets the
    solver build and own one.  The recurrence is stated in include/sprsolve_hip.h (sprs_svds_*) and runs in C++ on
    device-resident vectors and scalars (sprsolve_amd/csrc/svds.hip, svds_fuse.hpp); the handle holds 2 ncv + 3 work vectors.
    Single GPU."""
    NAME = "svds"
    SAYS_WHY = True     # a distributed A, a wrong adjoint, ncv out of range

    def __init__(self, A, ncv=0, adjoint=None):
        ncv = int(ncv)
        if ncv < 0:
            raise ValueError("ncv must be >= 0")
        self.AH = adjoint               # borrowed
        self.shape = tuple(A.shape)
        self._create(A, adjoint.h if adjoint is not None else None, ncv)
        self.ncv = ncv or min(32, min(self.shape))

    @classmethod
    def new(cls, A, ncv=0, adjoint=None):
        return cls(A, ncv, adjoint)

    def default_v0(self):
        """The start vector of `solve(v0=None)`: min(rows, cols) entries."""
        return stream_vector(min(self.shape), self.dtype, 92)

    def solve(self, k, which="largest", v0=None, max_restarts=1000, tol=0.0, vectors=True):
        """-> (s, U, V, info): s the k singular values in the order of `which`, U of shape (k, rows) and V of shape (k, cols) with
        the singular vectors of s[c] in row c (both None with vectors=False), info = dict(res, nconv, restarts, matvecs) with res
        the absolute residual estimates.  tol = 0.0 selects 1e-10 (f64 / c64) or 1e-4 (f32 / c32); a triplet counts as converged at
        res <= tol * (the largest singular value seen).  v0: a host array or a device vector of min(rows, cols) entries (a device
        v0 takes the device entry point; the results come back as host arrays either way).  Raises SolverError:
        InsufficientIterNum after max_restarts cycles and BreakDown (a NaN, a zero v0, a rank-deficient operator, an invariant
        subspace of fewer than k dimensions) carry what was computed as .s, .U, .V and .info."""
        k = int(k)
        which, tol = which_and_tol(which, tol, self.s, WHICH)
        v0p, v0l, dev, _keep = in_vec(self.default_v0() if v0 is None else v0, self.dtype)
        st, vals, (U, V), res, (nconv, restarts, matvecs) = eig_call(
            self, "svds", dev, (k, which, v0p, v0l, int(max_restarts), tol), k, self.shape, vectors and k > 0, 3)
        info = dict(res=res, nconv=nconv, restarts=restarts, matvecs=matvecs)
        return eig_result(st, (vals, U, V, info), ("s", "U", "V", "info"), restarts, self.A.ctx.h)
