"""The conjugate-gradient recurrence of include/sprsolve_hip.h (sprs_cg_*) restated in numpy, op for op, in the dtype under
test: the checker of tests/test_cg_cpu.py and tests/test_gpu_cg.py.  Every vector op rounds once per element operation as
the library's kernels do (no fused multiply-add in numpy); only the sums (np.vdot, np.linalg.norm, the row sums of the
matrix product) associate differently, so nothing is compared bit for bit against it."""
from collections import namedtuple

import numpy as np

OK, INCOMPATIBLE_RHS_SIZE, INCOMPATIBLE_X_SIZE, INSUFFICIENT_ITER, BREAKDOWN, INVALID_PRECOND = 0, 1, 2, 3, 4, 5

Result = namedtuple("Result", "status its res x trace")     # trace: rows (its, r_norm, rho, alpha, beta)


def _matvec(indptr, indices, data):
    import scipy.sparse as sp
    n = indptr.size - 1
    M = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    return lambda v: (M @ v).astype(data.dtype, copy=False)


def cg(indptr, indices, data, rhs, x0, max_iter, tol, precond_diag=None):
    """-> Result.  data / rhs / x0 share the dtype under test; precond_diag (the matrix diagonal handed to DiagPrecond, real or
    of the dtype) or None.  `res` is what the library reports in *res_out."""
    T = np.dtype(data.dtype)
    R = np.dtype(np.float32 if T in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    n = indptr.size - 1
    rhs = np.asarray(rhs, dtype=T); x = np.array(x0, dtype=T)
    if rhs.size != n:
        return Result(INCOMPATIBLE_RHS_SIZE, 0, 0.0, x, [])
    if x.size != n:
        return Result(INCOMPATIBLE_X_SIZE, 0, 0.0, x, [])
    A = _matvec(indptr, indices, data)
    one = T.type(1)
    dinv = None
    if precond_diag is not None:
        d = np.asarray(precond_diag)
        dinv = (d.dtype.type(1) / d)                       # DiagPrecond::new: V::one() / v, in V
    norm2 = lambda v: R.type(np.linalg.norm(v))
    cdot = lambda a, b: T.type(np.vdot(a, b))              # sum conj(a_i) b_i
    trace = []

    rhs_norm = norm2(rhs)
    if rhs_norm <= np.finfo(R).eps:
        return Result(OK, 0, float(rhs_norm), np.zeros(n, T), trace)
    tol2 = R.type(tol) * rhs_norm
    r = A(x)
    r = rhs * one + r * (-one)
    r_norm = norm2(r)
    if r_norm <= tol2:
        return Result(OK, 0, float(r_norm / rhs_norm), x, trace)
    z = (r * dinv).astype(T) if dinv is not None else r
    p = z.copy()
    rho = cdot(r, z)
    with np.errstate(all="ignore"):
        for its in range(max_iter):
            q = A(p)
            pq = cdot(p, q)
            if not (pq.real > 0):
                return Result(BREAKDOWN, its, 0.0, x, trace)
            alpha = T.type(rho / pq)
            x = x + p * alpha
            r = r + q * (-alpha)
            r_norm = norm2(r)
            if r_norm <= tol2:
                return Result(OK, its + 1, float(r_norm / rhs_norm), x, trace)
            z = (r * dinv).astype(T) if dinv is not None else r
            rho_new = cdot(r, z)
            if dinv is not None and not (rho_new.real > 0):
                return Result(INVALID_PRECOND, its, float(rho_new.real), x, trace)
            beta = T.type(rho_new / rho)
            rho = rho_new
            p = z * one + p * beta
            trace.append((its, float(r_norm), complex(rho), complex(alpha), complex(beta)))
    return Result(INSUFFICIENT_ITER, max_iter, 0.0, x, trace)


def trace_array(trace):
    """The rows in the library's 8-double layout: [its, r_norm, re rho, im rho, re alpha, im alpha, re beta, im beta]."""
    return np.array([[t[0], t[1], t[2].real, t[2].imag, t[3].real, t[3].imag, t[4].real, t[4].imag] for t in trace]).reshape(-1, 8)


def dense(indptr, indices, data):
    n = indptr.size - 1
    M = np.zeros((n, n), dtype=data.dtype)
    M[np.repeat(np.arange(n), np.diff(indptr)), indices] = data
    return M
