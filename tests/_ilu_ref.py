"""ILU(0) as include/sprsolve_hip.h states it (sprs_ilu0_*), restated with plain loops in the scalar type under test: the checker
of tests/test_ilu_cpu.py and tests/test_gpu_ilu.py.  Every scalar operation rounds once in the type's precision; complex numbers
are (re, im) pairs worked component by component with csrc/scalar.hpp's naive formulas, so the factors and the two triangular
folds can be compared BIT FOR BIT with the library's.  CG and GMRES with a callable preconditioner follow (tests/_cg_ref.py and
tests/_gmres_ref.py take a diagonal, not a callable); their sums associate as numpy's do, so nothing is compared bit for bit
against those."""
from collections import namedtuple

import numpy as np

from _gmres_ref import _Ops, _matvec, _tree

OK, INCOMPATIBLE_RHS_SIZE, INCOMPATIBLE_X_SIZE, INSUFFICIENT_ITER, BREAKDOWN, INVALID_PRECOND = 0, 1, 2, 3, 4, 5
INVALID_ARGUMENT, ZERO_DIAGONAL = 7, 8

Factors = namedtuple("Factors", "status row val")            # row: the offending row of ZERO_DIAGONAL / INVALID_ARGUMENT, else -1


class Scalar:
    """The four operations of the statement on scalars of dtype T.  A real scalar is a Python float (f64: the same IEEE
    operations) or an np.float32; a complex one is a pair of those."""

    def __init__(self, dtype):
        self.T = np.dtype(dtype)
        self.cx = self.T.kind == "c"
        self.single = self.T in (np.dtype(np.float32), np.dtype(np.complex64))
        self.R = np.float32 if self.single else np.float64

    # ---- reals: one rounding per operation
    def _r(self, v):
        return np.float32(v) if self.single else float(v)

    def _div(self, a, b):
        with np.errstate(all="ignore"):
            q = self.R(a) / self.R(b)                        # (a Python float would raise on a zero divisor)
        return q if self.single else float(q)

    # ---- scalars of T
    def load(self, v):
        return (self._r(v.real), self._r(v.imag)) if self.cx else self._r(v)

    def store(self, s):
        return self.T.type(complex(s[0], s[1])) if self.cx else self.T.type(s)

    def zero(self):
        return (self._r(0.0), self._r(0.0)) if self.cx else self._r(0.0)

    def add(self, a, b):
        return (a[0] + b[0], a[1] + b[1]) if self.cx else a + b

    def sub(self, a, b):
        return (a[0] - b[0], a[1] - b[1]) if self.cx else a - b

    def mul(self, a, b):
        if not self.cx:
            return a * b
        return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])

    def div(self, a, b):
        if not self.cx:
            return self._div(a, b)
        n = b[0] * b[0] + b[1] * b[1]
        return (self._div(a[0] * b[0] + a[1] * b[1], n), self._div(a[1] * b[0] - a[0] * b[1], n))

    def bad_pivot(self, s):
        re, im = (s if self.cx else (s, 0.0))
        return not (np.isfinite(re) and np.isfinite(im)) or (re == 0 and im == 0)

    def vec_load(self, v):
        return [self.load(e) for e in np.asarray(v, dtype=self.T)]

    def vec_store(self, s):
        return np.array([self.store(e) for e in s], dtype=self.T)


def check_pattern(indptr, indices):
    """-> (status, row): INVALID_ARGUMENT at the first row whose columns are not strictly ascending, else ZERO_DIAGONAL at the
    smallest row without a stored diagonal, else (OK, -1)."""
    n = indptr.size - 1
    for i in range(n):
        c = indices[indptr[i]:indptr[i + 1]]
        if np.any(np.diff(c) <= 0):
            return INVALID_ARGUMENT, i
    for i in range(n):
        if i not in indices[indptr[i]:indptr[i + 1]]:
            return ZERO_DIAGONAL, i
    return OK, -1


def ilu0(indptr, indices, data):
    """The factorisation of the header, in place on a copy of `data` -> Factors (val: nnz values at the CSR positions, l_ik below
    the diagonal, u_ij on and above it; None unless status is OK)."""
    st, row = check_pattern(indptr, indices)
    if st != OK:
        return Factors(st, row, None)
    S = Scalar(data.dtype)
    n = indptr.size - 1
    ip = [int(v) for v in indptr]; ix = [int(v) for v in indices]
    a = S.vec_load(data)
    dpos = [ix.index(i, ip[i], ip[i + 1]) for i in range(n)]
    for i in range(n):
        end = ip[i + 1]
        for pk in range(ip[i], end):
            k = ix[pk]
            if k >= i:
                break
            l = S.div(a[pk], a[dpos[k]])
            a[pk] = l
            q, qe, pj = dpos[k] + 1, ip[k + 1], pk + 1
            while pj < end and q < qe:                       # columns j > k that rows i and k both store
                if ix[pj] == ix[q]:
                    a[pj] = S.sub(a[pj], S.mul(l, a[q])); pj += 1; q += 1
                elif ix[pj] < ix[q]:
                    pj += 1
                else:
                    q += 1
    for i in range(n):
        if S.bad_pivot(a[dpos[i]]):
            return Factors(ZERO_DIAGONAL, i, None)
    return Factors(OK, -1, S.vec_store(a))


def levels(indptr, indices):
    """-> (level, ulevel): level(i) = 1 + max level(k) over the stored k < i; ulevel(i) = 1 + max ulevel(j) over the stored
    j > i, from the last row down (0 where there is none)."""
    n = indptr.size - 1
    lv = np.zeros(n, np.int64); ul = np.zeros(n, np.int64)
    for i in range(n):
        for p in range(indptr[i], indptr[i + 1]):
            if indices[p] < i:
                lv[i] = max(lv[i], lv[indices[p]] + 1)
    for i in range(n - 1, -1, -1):
        for p in range(indptr[i], indptr[i + 1]):
            if indices[p] > i:
                ul[i] = max(ul[i], ul[indices[p]] + 1)
    return lv, ul


def level_counts(indptr, indices):
    lv, ul = levels(indptr, indices)
    return (int(lv.max()) + 1, int(ul.max()) + 1) if lv.size else (0, 0)


class Applier:
    """The two folds on factors `val` (as ilu0 returns them).  solve(which, v): 0 = U^-1 L^-1 v, 1 = L^-1 v, 2 = U^-1 v."""

    def __init__(self, indptr, indices, val):
        self.S = Scalar(val.dtype)
        self.n = indptr.size - 1
        self.ip = [int(v) for v in indptr]; self.ix = [int(v) for v in indices]
        self.a = self.S.vec_load(val)
        self.dpos = [self.ix.index(i, self.ip[i], self.ip[i + 1]) for i in range(self.n)]

    def _lower(self, r):
        S, ix, a = self.S, self.ix, self.a
        y = [None] * self.n
        for i in range(self.n):
            sigma = S.zero()
            for p in range(self.ip[i], self.dpos[i]):
                sigma = S.add(sigma, S.mul(a[p], y[ix[p]]))
            y[i] = S.sub(r[i], sigma)
        return y

    def _upper(self, y):
        S, ix, a = self.S, self.ix, self.a
        z = [None] * self.n
        for i in range(self.n - 1, -1, -1):
            sigma = S.zero()
            for p in range(self.dpos[i] + 1, self.ip[i + 1]):
                sigma = S.add(sigma, S.mul(a[p], z[ix[p]]))
            z[i] = S.div(S.sub(y[i], sigma), a[self.dpos[i]])
        return z

    def solve(self, which, v):
        s = self.S.vec_load(v)
        if which in (0, 1):
            s = self._lower(s)
        if which in (0, 2):
            s = self._upper(s)
        return self.S.vec_store(s)

    def __call__(self, v):
        return self.solve(0, v)


def jacobi(indptr, indices, data):
    """The callable of DiagPrecond<T, T::Real> on the matrix diagonal (real part): v -> v * (1 / d)."""
    rows = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    d = data[rows == indices].real
    dinv = d.dtype.type(1) / d
    return lambda v: (v * dinv).astype(v.dtype)


CgResult = namedtuple("CgResult", "status its res x trace")  # trace: rows (its, r_norm, rho, alpha, beta)


def cg(indptr, indices, data, rhs, x0, max_iter, tol, prec=None):
    """tests/_cg_ref.py's cg with the preconditioner as a callable (None: none)."""
    T = np.dtype(data.dtype)
    R = np.dtype(np.float32 if T in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    n = indptr.size - 1
    rhs = np.asarray(rhs, dtype=T); x = np.array(x0, dtype=T)
    A = _matvec(indptr, indices, data)
    one = T.type(1)
    norm2 = lambda v: R.type(np.linalg.norm(v))
    cdot = lambda a, b: T.type(np.vdot(a, b))
    trace = []
    rhs_norm = norm2(rhs)
    if rhs_norm <= np.finfo(R).eps:
        return CgResult(OK, 0, float(rhs_norm), np.zeros(n, T), trace)
    tol2 = R.type(tol) * rhs_norm
    r = A(x)
    r = rhs * one + r * (-one)
    r_norm = norm2(r)
    if r_norm <= tol2:
        return CgResult(OK, 0, float(r_norm / rhs_norm), x, trace)
    z = prec(r) if prec is not None else r
    p = z.copy()
    rho = cdot(r, z)
    with np.errstate(all="ignore"):
        for its in range(max_iter):
            q = A(p)
            pq = cdot(p, q)
            if not (pq.real > 0):
                return CgResult(BREAKDOWN, its, 0.0, x, trace)
            alpha = T.type(rho / pq)
            x = x + p * alpha
            r = r + q * (-alpha)
            r_norm = norm2(r)
            if r_norm <= tol2:
                return CgResult(OK, its + 1, float(r_norm / rhs_norm), x, trace)
            z = prec(r) if prec is not None else r
            rho_new = cdot(r, z)
            if prec is not None and not (rho_new.real > 0):
                return CgResult(INVALID_PRECOND, its, float(rho_new.real), x, trace)
            beta = T.type(rho_new / rho)
            rho = rho_new
            p = z * one + p * beta
            trace.append((its, float(r_norm), complex(rho), complex(alpha), complex(beta)))
    return CgResult(INSUFFICIENT_ITER, max_iter, 0.0, x, trace)


GmResult = namedtuple("GmResult", "status its res x trace")  # trace: rows (its, |g_{j+1}|, hn, R_jj, cs_j, s_j)


def gmres(indptr, indices, data, rhs, x0, max_iter, tol, restart=30, prec=None, sums="numpy"):
    """tests/_gmres_ref.py's gmres with the right preconditioner as a callable (None: none); sums="pairwise": its explicit
    pairwise tree in place of numpy's own summation."""
    T = np.dtype(data.dtype)
    R = np.dtype(np.float32 if T in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    n = indptr.size - 1
    m = 30 if restart == 0 else int(restart)
    rhs = np.asarray(rhs, dtype=T); x = np.array(x0, dtype=T)
    A = _matvec(indptr, indices, data)
    op = _Ops(T, R)
    one = T.type(1)
    if sums == "numpy":
        norm2 = lambda v: R.type(np.linalg.norm(v))
        cdot = lambda a, b: T.type(np.vdot(a, b))
    else:
        norm2 = lambda v: R.type(np.sqrt(_tree((v.real * v.real + v.imag * v.imag).astype(R))))
        cdot = lambda a, b: T.type(_tree((np.conj(a) * b).astype(T)))
    if prec is None:
        prec = lambda v: v
    trace = []

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
        return GmResult(OK, 0, float(rhs_norm), np.zeros(n, T), trace)
    tol2 = R.type(tol) * rhs_norm
    its = 0
    with np.errstate(all="ignore"):
        while True:
            v0 = A(x)
            v0 = rhs * one + v0 * (-one)
            beta = norm2(v0)
            if beta <= tol2:
                return GmResult(OK, its, float(beta / rhs_norm), x, trace)
            if its == max_iter:
                return GmResult(INSUFFICIENT_ITER, max_iter, 0.0, x, trace)
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
                    return GmResult(BREAKDOWN, its, 0.0, x, trace)
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
                if gabs <= tol2 or hn == 0 or its == max_iter:
                    k = j + 1
                    break
                V.append((w * R.type(R.type(1) / hn)).astype(T))
            x = update(x, V, Rm, g, k)
            gk = op.abs(g[k])
            if gk <= tol2:
                return GmResult(OK, its, float(gk / rhs_norm), x, trace)
            if its == max_iter:
                return GmResult(INSUFFICIENT_ITER, max_iter, 0.0, x, trace)
