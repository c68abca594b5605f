"""IDR(s) for general (non-symmetric) operators (no reference analogue)."""
from . import _lib
from ._solver import _SolverBase, applied_prefix


class IDRS(_SolverBase):
    """`IDRS.new(A, size, s=4)`: the bi-orthogonal IDR(s) of van Gijzen & Sonneveld, right-preconditioned: a short recurrence on
    3 s + 4 work vectors with a fixed cost per product with A and no restart; s is at most 8 (0 means 4) and at most `size`.
    The shadow space is the generators' uniform streams 200 + .., orthonormalised once at creation; every dot product of the
    recurrence is accumulated in double, in single precision too.  The recurrence is stated in
    include/sprsolve_hip.h (sprs_idrs_*) and runs in C++ on device-resident vectors and scalars (sprsolve_amd/csrc/idrs.hip,
    idrs_fuse.hpp).  Conventions as BiCGStab's: relative residual against |rhs|, x in/out; `iters` counts products with A
    after the initial residual.  One mode: `set_mode('literal')` is refused.  Single GPU."""
    KIND = _lib.SOLVER_IDRS
    NAME = "idrs"
    SAYS_WHY = True     # s out of range, a distributed A

    def __init__(self, A, size, s=4):
        s = int(s)
        if s < 0:
            raise ValueError("s must be >= 0")
        self.s_dim = s or 4
        super().__init__(A, size, s)

    @classmethod
    def new(cls, A, size, s=4):
        return cls(A, size, s)

    def solve(self, rhs, x, max_iter, tol):
        """Returns (iters, relative residual); raises SolverError (BreakDown: a zero pivot, |A vh| = 0 or a norm that is not finite)."""
        return self._solve(None, rhs, x, max_iter, tol, False)

    def precond_solve(self, precond, rhs, x, max_iter, tol):
        """Preconditioned from the right by a `DiagPrecond` (Jacobi), an `ILU0`, an `AMG` or an `FSAI`: the residual it reports is the recursive one."""
        prefix = applied_prefix(precond)
        if prefix == "bjacobi":                              # (the library has no sprs_bjacobi_idrs_* entry points)
            raise TypeError("IDRS does not take a BlockJacobi: precond must be a DiagPrecond, ILU0, AMG or FSAI")
        return self._solve(precond, rhs, x, max_iter, tol, True, prefix=prefix)
