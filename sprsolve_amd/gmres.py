"""Restarted GMRES for general (non-symmetric) operators (no reference analogue)."""
from . import _lib
from ._solver import _SolverBase, applied_prefix


class GMRES(_SolverBase):
    """`GMRES.new(A, size, restart=30)`: GMRES(restart), right-preconditioned, classical Gram-Schmidt applied twice, Givens
    rotations; restart is at most 64 (0 means 30).  The recurrence is stated in include/sprsolve_hip.h (sprs_gmres_*) and runs in
    C++ on device-resident vectors and scalars (sprsolve_amd/csrc/gmres.hip, gmres_fuse.hpp); the handle holds restart + 4
    work vectors.  Conventions as BiCGStab's: relative residual against |rhs|, x in/out; `iters` counts Arnoldi steps."""
    KIND = _lib.SOLVER_GMRES
    NAME = "gmres"

    def __init__(self, A, size, restart=30):
        restart = int(restart)
        if restart < 0:
            raise ValueError("restart must be >= 0")
        self.restart = restart or 30
        super().__init__(A, size, restart)

    @classmethod
    def new(cls, A, size, restart=30):
        return cls(A, size, restart)

    def solve(self, rhs, x, max_iter, tol):
        """Returns (iters, relative residual); raises SolverError (BreakDown only where a norm is NaN)."""
        return self._solve(None, rhs, x, max_iter, tol, False)

    def precond_solve(self, precond, rhs, x, max_iter, tol):
        """Preconditioned from the right by a `DiagPrecond` (Jacobi), an `ILU0`, an `AMG`, an `FSAI` or a `BlockJacobi`: the residual it reports is the true one's estimate."""
        return self._solve(precond, rhs, x, max_iter, tol, True, prefix=applied_prefix(precond))
