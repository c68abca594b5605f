"""The restarted-GMRES recurrence of include/sprsolve_hip.h (sprs_gmres_*) restated in numpy, op for op, in the dtype under
test: the checker of tests/test_gmres_cpu.py and tests/test_gpu_gmres.py.  Every vector op and every scalar op rounds once
per operation as the library's do (no fused multiply-add in numpy; complex products and quotients are spelled out in the
library's naive formulas); only the sums (the dot products, the norms, the row sums of the matrix product) associate
differently, so nothing is compared bit for bit against it.  `sums="pairwise"` replaces numpy's own summation by an explicit
pairwise tree: the two orders bracket what a change of summation order does to the iterates."""
from collections import namedtuple

import numpy as np

OK, INCOMPATIBLE_RHS_SIZE, INCOMPATIBLE_X_SIZE, INSUFFICIENT_ITER, BREAKDOWN, INVALID_PRECOND = 0, 1, 2, 3, 4, 5
MAX_RESTART = 64

# trace: rows (its, |g_{j+1}|, hn, R_jj, cs_j, s_j); xs (keep_iterates): the x each step WOULD give, for the CPU tests
Result = namedtuple("Result", "status its res x trace xs")


def _matvec(indptr, indices, data):
    import scipy.sparse as sp
    n = indptr.size - 1
    M = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    return lambda v: (M @ v).astype(data.dtype, copy=False)


def _tree(v):
    v = np.asarray(v)
    while v.size > 1:
        if v.size & 1:
            v = np.concatenate([v, np.zeros(1, v.dtype)])
        v = v[0::2] + v[1::2]
    return v[0] if v.size else v.dtype.type(0)


class _Ops:
    """The library's scalar operations (csrc/scalar.hpp) on numpy scalars of the dtype under test."""

    def __init__(self, T, R):
        self.T, self.R, self.cx = T, R, T.kind == "c"

    def mul(self, a, b):
        if not self.cx:
            return self.T.type(a * b)
        R = self.R.type
        ar, ai, br, bi = R(a.real), R(a.imag), R(b.real), R(b.imag)
        return self.T.type(complex(R(R(ar * br) - R(ai * bi)), R(R(ar * bi) + R(ai * br))))

    def div(self, a, b):
        if not self.cx:
            return self.T.type(a / b)
        R = self.R.type
        ar, ai, br, bi = R(a.real), R(a.imag), R(b.real), R(b.imag)
        nn = R(R(br * br) + R(bi * bi))
        return self.T.type(complex(R(R(R(ar * br) + R(ai * bi)) / nn), R(R(R(ai * br) - R(ar * bi)) / nn)))

    def mulr(self, a, r):
        if not self.cx:
            return self.T.type(a * r)
        R = self.R.type
        return self.T.type(complex(R(R(a.real) * r), R(R(a.imag) * r)))

    def add(self, a, b):
        return self.T.type(a + b)

    def sub(self, a, b):
        return self.T.type(a - b)

    def abs(self, a):
        return self.R.type(np.hypot(self.R.type(a.real), self.R.type(a.imag))) if self.cx else self.R.type(abs(a))

    def nconj(self, a):
        return self.T.type(-np.conj(a))


def gmres(indptr, indices, data, rhs, x0, max_iter, tol, restart=30, precond_diag=None, sums="numpy", keep_iterates=False):
    """-> Result.  data / rhs / x0 share the dtype under test; precond_diag (the matrix diagonal handed to DiagPrecond, real or
    of the dtype) or None.  `res` is what the library reports in *res_out."""
    T = np.dtype(data.dtype)
    R = np.dtype(np.float32 if T in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    n = indptr.size - 1
    m = 30 if restart == 0 else int(restart)
    if m > MAX_RESTART:
        raise ValueError("restart > %d" % MAX_RESTART)
    rhs = np.asarray(rhs, dtype=T); x = np.array(x0, dtype=T)
    if rhs.size != n:
        return Result(INCOMPATIBLE_RHS_SIZE, 0, 0.0, x, [], [])
    if x.size != n:
        return Result(INCOMPATIBLE_X_SIZE, 0, 0.0, x, [], [])
    A = _matvec(indptr, indices, data)
    op = _Ops(T, R)
    one = T.type(1)
    dinv = None
    if precond_diag is not None:
        d = np.asarray(precond_diag)
        dinv = (d.dtype.type(1) / d)                       # DiagPrecond::new: V::one() / v, in V
    if sums == "numpy":
        norm2 = lambda v: R.type(np.linalg.norm(v))
        cdot = lambda a, b: T.type(np.vdot(a, b))          # sum conj(a_i) b_i
    else:
        norm2 = lambda v: R.type(np.sqrt(_tree((v.real * v.real + v.imag * v.imag).astype(R))))
        cdot = lambda a, b: T.type(_tree((np.conj(a) * b).astype(T)))
    prec = (lambda v: (v * dinv).astype(T)) if dinv is not None else (lambda v: v)
    trace, xs = [], []

    def update(x, V, Rm, g, k):
        y = np.zeros(k, T)
        for i in range(k - 1, -1, -1):
            t = g[i]
            for l in range(i + 1, k):
                t = op.sub(t, op.mul(Rm[i, l], y[l]))
            y[i] = op.div(t, Rm[i, i])
        u = np.zeros(n, T)
        for i in range(k):
            u = u + V[i] * y[i]
        u = prec(u)
        return x + u * one

    rhs_norm = norm2(rhs)
    if rhs_norm <= np.finfo(R).eps:
        return Result(OK, 0, float(rhs_norm), np.zeros(n, T), trace, xs)
    tol2 = R.type(tol) * rhs_norm
    its = 0
    with np.errstate(all="ignore"):
        while True:
            v0 = A(x)
            v0 = rhs * one + v0 * (-one)
            beta = norm2(v0)
            if beta <= tol2:
                return Result(OK, its, float(beta / rhs_norm), x, trace, xs)
            if its == max_iter:
                return Result(INSUFFICIENT_ITER, max_iter, 0.0, x, trace, xs)
            V = [(v0 * R.type(R.type(1) / beta)).astype(T)]
            g = np.zeros(m + 1, T); g[0] = T.type(beta)
            cs = np.zeros(m, R); sn = np.zeros(m, T)
            Rm = np.zeros((m, m), T)
            k = m
            for j in range(m):
                w = A(prec(V[j]))
                h = np.array([cdot(V[i], w) for i in range(j + 1)], T)
                for i in range(j + 1):
                    w = w + V[i] * T.type(-h[i])
                c2 = np.array([cdot(V[i], w) for i in range(j + 1)], T)
                for i in range(j + 1):
                    w = w + V[i] * T.type(-c2[i])
                h = np.concatenate([(h + c2).astype(T), np.zeros(1, T)])
                hn = norm2(w)
                if not (hn >= 0):
                    return Result(BREAKDOWN, its, 0.0, x, trace, xs)
                for i in range(j):
                    t = op.add(op.mulr(h[i], cs[i]), op.mul(sn[i], h[i + 1]))
                    h[i + 1] = op.add(op.mul(op.nconj(sn[i]), h[i]), op.mulr(h[i + 1], cs[i]))
                    h[i] = t
                a = h[j]
                aa = op.abs(a)
                dd = R.type(np.sqrt(R.type(R.type(aa * aa) + R.type(hn * hn))))
                if aa == 0:
                    cs[j] = 0; sn[j] = one
                else:
                    cs[j] = R.type(aa / dd)
                    sn[j] = op.mulr(a, R.type(R.type(hn / dd) / aa))
                h[j] = op.add(op.mulr(a, cs[j]), op.mulr(sn[j], hn))
                Rm[: j + 1, j] = h[: j + 1]
                g[j + 1] = op.mul(op.nconj(sn[j]), g[j])
                g[j] = op.mulr(g[j], cs[j])
                its += 1
                gabs = op.abs(g[j + 1])
                trace.append((its, float(gabs), float(hn), complex(h[j]), float(cs[j]), complex(sn[j])))
                if keep_iterates:
                    xs.append(update(x, V, Rm, g, j + 1))
                if gabs <= tol2 or hn == 0 or its == max_iter:
                    k = j + 1
                    break
                V.append((w * R.type(R.type(1) / hn)).astype(T))
            x = update(x, V, Rm, g, k)
            gk = op.abs(g[k])
            if gk <= tol2:
                return Result(OK, its, float(gk / rhs_norm), x, trace, xs)
            if its == max_iter:
                return Result(INSUFFICIENT_ITER, max_iter, 0.0, x, trace, xs)


def trace_array(trace):
    """The rows in the library's 8-double layout: [its, |g_{j+1}|, hn, re R_jj, im R_jj, cs_j, re s_j, im s_j]."""
    return np.array([[t[0], t[1], t[2], t[3].real, t[3].imag, t[4], t[5].real, t[5].imag] for t in trace]).reshape(-1, 8)


def dense(indptr, indices, data):
    n = indptr.size - 1
    M = np.zeros((n, n), dtype=data.dtype)
    M[np.repeat(np.arange(n), np.diff(indptr)), indices] = data
    return M
