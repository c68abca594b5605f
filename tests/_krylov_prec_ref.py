"""BiCGStab and MINRES with the preconditioner as a callable, restated in numpy op for op after the literal modes of
csrc/bicgstab.hip and csrc/minres.hip (run_literal), in the dtype under test: the checker of tests/test_krylov_prec_cpu.py and
tests/test_gpu_krylov_prec.py.  Every vector op and every scalar op rounds once per operation as the library's do (complex
products and quotients in csrc/scalar.hpp's naive formulas, tests/_gmres_ref.py's _Ops); only the sums (dot products, norms, the
row sums of the matrix product) associate differently, so nothing is compared bit for bit against it.  sums="pairwise" replaces
numpy's own summation by an explicit pairwise tree: the two orders bracket what a change of summation order does.

prec: None, or a callable v -> M v (tests/_ilu_ref.py's jacobi and Applier, tests/_ilu_sweeps_ref.py's Sweeps,
tests/_amg_ref.py's Applier).  Trace rows are the library's 8 doubles:
  BiCGStab  (its, |r| at the top of the iteration (row 0: |r0|), re rho, im rho, re alpha, im alpha, re w, im w)
  MINRES    (its, beta_new, re alpha, im alpha, re c, im c, s, res_norm)"""
from collections import namedtuple

import numpy as np

from _gmres_ref import _Ops, _matvec, _tree

OK, INCOMPATIBLE_RHS_SIZE, INCOMPATIBLE_X_SIZE, INSUFFICIENT_ITER, BREAKDOWN, INVALID_PRECOND = 0, 1, 2, 3, 4, 5

# events: BiCGStab: the iterations that took the restart branch; MINRES: [(its, re b2, im b2)] of every preconditioned step
Result = namedtuple("Result", "status its res x trace events")


def _setup(data, rhs, x0, sums):
    T = np.dtype(data.dtype)
    R = np.dtype(np.float32 if T in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    rhs = np.asarray(rhs, dtype=T); x = np.array(x0, dtype=T)
    if sums == "numpy":
        norm2 = lambda v: R.type(np.linalg.norm(v))
        cdot = lambda a, b: T.type(np.vdot(a, b))
    elif sums == "pairwise":
        norm2 = lambda v: R.type(np.sqrt(_tree((v.real * v.real + v.imag * v.imag).astype(R))))
        cdot = lambda a, b: T.type(_tree((np.conj(a) * b).astype(T)))
    else:
        raise ValueError(sums)
    return T, R, rhs, x, norm2, cdot


def _trace(rows):
    return np.array(rows, dtype=np.float64).reshape(-1, 8)


def bicgstab(indptr, indices, data, rhs, x0, max_iter, tol, prec=None, sums="numpy"):
    """BicgStab<T>::run_literal (bicg_stab.rs:35-366, right-preconditioned): y = M p before v = A y, z = M s before t = A z."""
    T, R, rhs, x, norm2, cdot = _setup(data, rhs, x0, sums)
    n = indptr.size - 1
    A = _matvec(indptr, indices, data)
    op = _Ops(T, R)
    one = T.type(1); eps = np.finfo(R).eps
    axpy = lambda a, xx, yy: (yy + xx * a).astype(T)            # launch_axpy: y = y + x a
    rows, restarts = [], []

    def row(its, rn, rho, alpha, w):
        rows.append([its, float(rn), rho.real, rho.imag, alpha.real, alpha.imag, w.real, w.imag])

    def residual(x):
        r = A(x)
        return axpy(-one, rhs, r)                              # r = A x - rhs, the reference's sign

    with np.errstate(all="ignore"):
        rhs_norm = norm2(rhs)
        if rhs_norm <= eps:
            return Result(OK, 0, float(rhs_norm), np.zeros(n, T), _trace(rows), restarts)
        tol2 = R.type(R.type(tol) * rhs_norm)
        r = residual(x)
        r0 = r.copy()
        r0_norm = norm2(r0)
        if r0_norm <= tol2:
            return Result(OK, 0, float(r0_norm / rhs_norm), x, _trace(rows), restarts)
        r0_norm_tol = R.type(r0_norm * eps)
        r0_norm_tol = R.type(r0_norm_tol * r0_norm_tol)
        rho = T.type(R.type(r0_norm * r0_norm))
        p = r.copy()
        y = prec(p) if prec is not None else p
        v = A(y)
        alpha = op.div(rho, cdot(r0, v))
        r = axpy(-alpha, v, r)
        sz = prec(r) if prec is not None else r
        t = A(sz)
        tt = cdot(t, t)
        w = op.div(cdot(t, r), tt) if tt.real > 0 else T.type(0)
        x = axpy(-alpha, y, x)
        x = axpy(-w, sz, x)
        r = axpy(-w, t, r)
        row(0, r0_norm, rho, alpha, w)
        for its in range(1, max_iter):
            r_norm = norm2(r)
            if r_norm <= tol2:
                return Result(OK, its, float(r_norm / rhs_norm), x, _trace(rows), restarts)
            rho_old = rho
            rho = cdot(r0, r)
            if op.abs(rho) < r0_norm_tol:                      # :131-145
                restarts.append(its)
                r = residual(x)
                r0 = r.copy()
                rn = norm2(r)
                rho = T.type(R.type(rn * rn))
                r0_norm_tol = R.type(R.type(rho.real * eps) * eps)
            beta = op.mul(op.div(rho, rho_old), op.div(alpha, w))
            p = (v * op.mul(T.type(-beta), w) + p * beta).astype(T)     # launch_axpby(-beta w, v, beta, p)
            p = axpy(one, r, p)
            y = prec(p) if prec is not None else p
            v = A(y)
            tmp = cdot(r0, v)
            if op.abs(tmp) <= 0:
                return Result(BREAKDOWN, its, 0.0, x, _trace(rows), restarts)
            alpha = op.div(rho, tmp)
            r = axpy(-alpha, v, r)
            sz = prec(r) if prec is not None else r
            t = A(sz)
            tt = cdot(t, t)
            w = op.div(cdot(t, r), tt) if tt.real > 0 else T.type(0)
            x = axpy(-alpha, y, x)
            x = axpy(-w, sz, x)
            r = axpy(-w, t, r)
            row(its, r_norm, rho, alpha, w)
    return Result(INSUFFICIENT_ITER, max_iter, 0.0, x, _trace(rows), restarts)


def minres(indptr, indices, data, rhs, x0, max_iter, tol, prec=None, sums="numpy"):
    """MinRes<T>::run_literal (minres.rs:31-341) for a real symmetric / complex Hermitian A and a Hermitian positive-definite M.
    `its` is 0-based, as upstream.  INVALID_PRECOND: res = re(b2), by the reference's rule (minres.rs:279-287)."""
    T, R, rhs, x, norm2, cdot = _setup(data, rhs, x0, sums)
    n = indptr.size - 1
    A = _matvec(indptr, indices, data)
    op = _Ops(T, R)
    one = T.type(1); eps = np.finfo(R).eps
    r_ = R.type
    axpy = lambda a, xx, yy: (yy + xx * a).astype(T)
    rscale = lambda a, xx: (xx * r_(a)).astype(T)              # launch_rscale: a real factor on both components
    fromr = lambda a: T.type(r_(a))
    rows, b2s = [], []
    pc = prec is not None

    def invalid(b2):
        return r_(b2.real) < eps or r_(b2.imag) > r_(eps * r_(b2.real))

    with np.errstate(all="ignore"):
        rhs_norm = norm2(rhs)
        if rhs_norm <= eps:
            return Result(OK, 0, float(rhs_norm), np.zeros(n, T), _trace(rows), b2s)
        threshold = r_(r_(tol) * rhs_norm)
        cc, c_old, eta = one, one, one
        s, s_old = r_(0), r_(0)
        v_new = rhs.copy()
        v_old = A(x)
        v_new = axpy(-one, v_old, v_new)
        res_norm = norm2(v_new)
        w = w_new = None
        if pc:
            w_new = prec(v_new)
            b2 = cdot(v_new, w_new)
            b2s.append((-1, float(b2.real), float(b2.imag)))
            if invalid(b2):
                return Result(INVALID_PRECOND, 0, float(b2.real), x, _trace(rows), b2s)
            beta_new = r_(np.sqrt(r_(b2.real)))
            v_new = rscale(r_(1) / beta_new, v_new)
            w_new = rscale(r_(1) / beta_new, w_new)
        else:
            beta_new = res_norm
            v_new = rscale(r_(1) / beta_new, v_new)
        beta_one = beta_new
        v = np.zeros(n, T); p_old = np.zeros(n, T); p = np.zeros(n, T); p_oold = np.zeros(n, T)
        for its in range(max_iter):
            beta = beta_new
            v_old, v, v_new = v, v_new, v_old
            if pc:
                w, w_new = w_new, w
                q = w
            else:
                q = v
            v_new = A(q)
            alpha = cdot(q, v_new)
            v_new = axpy(fromr(-beta), v_old, v_new)
            v_new = axpy(T.type(-alpha), v, v_new)
            if pc:
                w_new = prec(v_new)
                b2 = cdot(v_new, w_new)
                b2s.append((its, float(b2.real), float(b2.imag)))
                if invalid(b2):
                    return Result(INVALID_PRECOND, its, float(b2.real), x, _trace(rows), b2s)
                beta_new = r_(np.sqrt(r_(b2.real)))
                v_new = rscale(r_(1) / beta_new, v_new)
                w_new = rscale(r_(1) / beta_new, w_new)
            else:
                beta_new = norm2(v_new)
                v_new = rscale(r_(1) / beta_new, v_new)
            r3 = r_(s_old * beta)
            tr = op.mulr(c_old, beta)
            r2 = op.add(op.mulr(alpha, s), op.mul(cc, tr))
            r1_hat = op.sub(op.mul(cc, alpha), op.mulr(tr, s))
            ssq = r_(r_(r1_hat.real) * r_(r1_hat.real)) + r_(r_(r1_hat.imag) * r_(r1_hat.imag)) if op.cx else r_(r1_hat * r1_hat)
            r1_inv = r_(r_(1) / r_(np.sqrt(r_(r_(ssq) + r_(beta_new * beta_new)))))
            c_old, s_old = cc, s
            cc = op.mulr(r1_hat, r1_inv)
            s = r_(beta_new * r1_inv)
            p_oold, p_old, p = p_old, p, p_oold
            p = q.copy()
            p = axpy(T.type(-r2), p_old, p)
            p = axpy(fromr(-r3), p_oold, p)
            p = rscale(r1_inv, p)
            x = axpy(op.mulr(op.mul(cc, eta), beta_one), p, x)
            res_norm = r_(res_norm * op.abs(fromr(s)))
            rows.append([its, float(beta_new), alpha.real, alpha.imag, cc.real, cc.imag, float(s), float(res_norm)])
            if res_norm < threshold:
                return Result(OK, its, float(res_norm / rhs_norm), x, _trace(rows), b2s)
            eta = op.mulr(eta, r_(-s))
    return Result(INSUFFICIENT_ITER, max_iter, 0.0, x, _trace(rows), b2s)
