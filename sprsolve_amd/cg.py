"""Conjugate gradients for Hermitian positive-definite operators (no reference analogue)."""
from . import _lib
from ._solver import _SolverBase, applied_prefix


class CG(_SolverBase):
    """`CG.new(A, size)`; A must be Hermitian positive definite (not checked).  The recurrence is stated in
    include/sprsolve_hip.h (sprs_cg_*) and runs in C++ on device-resident vectors and scalars
    (sprsolve_amd/csrc/cg.hip, cg_fuse.hpp).  Conventions as BiCGStab's: relative residual against |rhs|, x in/out."""
    KIND = _lib.SOLVER_CG
    NAME = "cg"

    def solve(self, rhs, x, max_iter, tol):
        """Returns (iters, relative residual); raises SolverError (BreakDown where conj(p).A p is not positive)."""
        return self._solve(None, rhs, x, max_iter, tol, False)

    def precond_solve(self, precond, rhs, x, max_iter, tol):
        """Preconditioned by a `DiagPrecond` (Jacobi), an `ILU0`, an `AMG`, an `FSAI` or a `BlockJacobi`; InvalidPreconditioner where conj(r).M^-1 r is not positive."""
        return self._solve(precond, rhs, x, max_iter, tol, True, prefix=applied_prefix(precond))
