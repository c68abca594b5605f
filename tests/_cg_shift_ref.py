"""The multi-shift conjugate-gradient recurrence of include/sprsolve_hip.h (sprs_cgshift_*) restated in numpy, op for op, in the
dtype under test, with the zeta scalars and the column coefficients as Python floats (doubles, as in the library): the checker of
tests/test_cg_shift_cpu.py and tests/test_gpu_cg_shift.py.  Only the sums associate differently (see _cg_ref.py), so nothing is
compared bit for bit against it."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_ref as ref  # noqa: E402

OK, INSUFFICIENT_ITER, BREAKDOWN = ref.OK, ref.INSUFFICIENT_ITER, ref.BREAKDOWN


def cg_shift(indptr, indices, data, rhs, shifts, max_iter, tol):
    """-> (its, res, status, X): arrays of m = len(shifts) entries and the (m, n) block of solutions of (A + shifts[j] I) x = rhs."""
    T = np.dtype(data.dtype)
    R = np.dtype(np.float32 if T in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    n = indptr.size - 1
    m = len(shifts)
    A = ref._matvec(indptr, indices, data)
    rhs = np.asarray(rhs, dtype=T)
    one = T.type(1)
    its = np.zeros(m, np.int64); res = np.zeros(m, R); status = np.zeros(m, np.int32)
    X = np.zeros((m, n), T)

    rhs_norm = R.type(np.linalg.norm(rhs))
    if rhs_norm <= np.finfo(R).eps:
        res[:] = rhs_norm
        return its, res, status, X
    tol2 = R.type(tol) * rhs_norm
    r = rhs.copy()
    if float(rhs_norm) <= float(tol2):
        res[:] = R.type(float(rhs_norm) / float(rhs_norm))
        return its, res, status, X
    p = r.copy()
    rho = T.type(np.vdot(r, r))
    P = [r.copy() for _ in range(m)]
    z = [1.0] * m; zp = [1.0] * m
    a_old, b_old = 1.0, 0.0
    running = [True] * m
    status[:] = INSUFFICIENT_ITER; its[:] = max_iter
    with np.errstate(all="ignore"):
        for it in range(max_iter):
            q = A(p)
            pq = T.type(np.vdot(p, q))
            if not (pq.real > 0):
                for j in range(m):
                    if running[j]:
                        status[j], its[j], running[j] = BREAKDOWN, it, False
                break
            alpha = T.type(rho / pq)
            a = float(alpha.real)
            zn = [0.0] * m
            for j in range(m):
                if not running[j]:
                    continue
                den = a * b_old * (zp[j] - z[j]) + zp[j] * a_old * (1.0 + float(shifts[j]) * a)
                zn[j] = z[j] * zp[j] * a_old / den if den != 0.0 else math.nan
                if den == 0.0 or not math.isfinite(zn[j]):
                    status[j], its[j], running[j] = BREAKDOWN, it, False
            if not any(running):
                break
            r = r + q * (-alpha)
            sN = R.type(np.vdot(r, r).real)
            r_norm = R.type(np.sqrt(sN))
            rho_new = T.type(sN)
            beta = T.type(rho_new / rho)
            b = float(beta.real)
            for j in range(m):
                if not running[j]:
                    continue
                t = zn[j] / z[j]
                X[j] = X[j] + P[j] * R.type(a * t)
                w = abs(zn[j]) * float(r_norm)
                if w <= float(tol2):
                    status[j], its[j], res[j], running[j] = OK, it + 1, R.type(w / float(rhs_norm)), False
                else:
                    P[j] = r * R.type(zn[j]) + P[j] * R.type(b * (t * t))
                    zp[j], z[j] = z[j], zn[j]
            p = r * one + p * beta
            rho = rho_new
            a_old, b_old = a, b
            if not any(running):
                break
    return its, res, status, X


def shifted(indptr, indices, data, sigma):
    """The CSR arrays of A + sigma I (A stores its whole diagonal)."""
    d = data.copy()
    diag = np.repeat(np.arange(indptr.size - 1), np.diff(indptr)) == indices
    assert np.count_nonzero(diag) == indptr.size - 1
    d[diag] = d[diag] + data.dtype.type(sigma)
    return d
