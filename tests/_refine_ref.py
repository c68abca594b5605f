"""The mixed-precision refinement recurrence of include/sprsolve_hip.h (sprs_refine_*) restated in numpy, op for op: the checker
of tests/test_refine_cpu.py and tests/test_gpu_refine.py.  The outer loop runs in the dtype H of the data (f64 / c64); the inner
solves are tests/_cg_ref.py / tests/_gmres_ref.py in L (f32 / c32) on `data.astype(L)`.  Every vector op rounds once per element
operation as the library's kernels do (a real scale multiplies the components of a complex element: mul_real); only the sums
associate differently, so iterates are never compared bit for bit against it.

One more difference, of the same size: the library's inner preconditioner is fl_L(1 / d) (the stored reciprocal rounded to L),
the inner checkers form 1 / fl_L(d) from the diagonal they are handed.  The two differ by at most one unit in the last place of
L per entry."""
from collections import namedtuple

import numpy as np

import _cg_ref
import _gmres_ref

OK, INCOMPATIBLE_RHS_SIZE, INCOMPATIBLE_X_SIZE, INSUFFICIENT_ITER, BREAKDOWN, INVALID_PRECOND = 0, 1, 2, 3, 4, 5

# outer: steps made; inner: the inner solves' iteration counts, one per step; res: what the library reports in *res_out;
# hist: the relative residual found at the top of every step; xs (keep_iterates): x after every update
Result = namedtuple("Result", "status outer inner res x hist xs")

LOW = {np.dtype(np.float64): np.dtype(np.float32), np.dtype(np.complex128): np.dtype(np.complex64)}


def _mulr(v, a):
    """v * a for a real a: per component (the library's smulr), also where v is complex."""
    if v.dtype.kind != "c":
        return v * a
    R = np.dtype(np.float32 if v.dtype == np.complex64 else np.float64)
    return (np.ascontiguousarray(v).view(R) * R.type(a)).view(v.dtype)


def demote_scaled(v, scale, L):
    """fl_L(v * scale): the product rounded in H::Real, then one rounding to L per component."""
    with np.errstate(over="ignore", invalid="ignore"):
        return _mulr(v, scale).astype(L)


def axpy_promoted(x, e, alpha):
    """x + fl_H(e) * alpha: the product rounded, then the sum."""
    with np.errstate(over="ignore", invalid="ignore"):
        return x + _mulr(e.astype(x.dtype), alpha)


def refine(indptr, indices, data, rhs, x0, max_outer, tol, inner_max_iter, inner_tol, inner="cg", restart=30, precond_diag=None,
           keep_iterates=False):
    """-> Result.  data / rhs / x0 are f64 or c64; precond_diag (the matrix diagonal handed to DiagPrecond, real or of the
    dtype) or None."""
    H = np.dtype(data.dtype)
    L = LOW[H]
    n = indptr.size - 1
    rhs = np.asarray(rhs, dtype=H); x = np.array(x0, dtype=H)
    if rhs.size != n:
        return Result(INCOMPATIBLE_RHS_SIZE, 0, [], 0.0, x, [], [])
    if x.size != n:
        return Result(INCOMPATIBLE_X_SIZE, 0, [], 0.0, x, [], [])
    A = _cg_ref._matvec(indptr, indices, data)
    data_lo = data.astype(L)
    pd_lo = None
    if precond_diag is not None:
        d = np.asarray(precond_diag)
        pd_lo = d.astype(np.complex64 if d.dtype.kind == "c" else np.float32)
    one = H.type(1)
    inner_counts, hist, xs = [], [], []

    b_norm = np.float64(np.linalg.norm(rhs))
    if b_norm <= np.finfo(np.float64).eps:
        return Result(OK, 0, inner_counts, float(b_norm), np.zeros(n, H), hist, xs)
    k = 0
    with np.errstate(all="ignore"):
        while True:
            r = rhs * one + A(x) * (-one)
            r_norm = np.float64(np.linalg.norm(r))
            res = np.float64(r_norm / b_norm)
            hist.append(float(res))
            if res <= tol:
                return Result(OK, k, inner_counts, float(res), x, hist, xs)
            if not np.isfinite(r_norm):
                return Result(BREAKDOWN, k, inner_counts, float(res), x, hist, xs)
            if k == max_outer:
                return Result(INSUFFICIENT_ITER, k, inner_counts, float(res), x, hist, xs)
            s = r_norm
            rl = demote_scaled(r, np.float64(1.0) / s, L)
            e0 = np.zeros(n, L)
            if inner == "cg":
                o = _cg_ref.cg(indptr, indices, data_lo, rl, e0, inner_max_iter, np.float32(inner_tol), precond_diag=pd_lo)
            else:
                o = _gmres_ref.gmres(indptr, indices, data_lo, rl, e0, inner_max_iter, np.float32(inner_tol), restart=restart,
                                     precond_diag=pd_lo)
            inner_counts.append(o.its)
            if o.status not in (OK, INSUFFICIENT_ITER):
                return Result(o.status, k, inner_counts, float(res), x, hist, xs)
            x = axpy_promoted(x, o.x, s)
            if keep_iterates:
                xs.append(x.copy())
            k += 1
