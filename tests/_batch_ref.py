"""The on-chip batch solvers as include/sprsolve_hip.h states them (sprs_batch_*), restated on the CPU in the scalar type under
test: the checker of tests/test_batch_cpu.py and tests/test_gpu_batch.py.  Every scalar operation rounds once in the type's
precision — tests/_ilu_ref.py's `Scalar`, whose four operations are plain operators and so work on numpy arrays of the type's real
precision as they do on single scalars; a complex vector is a pair of real arrays, worked component by component with the naive
formulas.  Sums over rows are taken in the stated order for B threads: thread t folds from +0 over i = t, t + B, .. ascending, the
butterfly v[l] += v[l + off], off = 32 .. 1, inside each wavefront of 64, then the B / 64 wavefronts left to right.  The row
fold is sigma = +0, then sigma + a_ij x_j over the stored j ascending.  So the product and both recurrences can be compared BIT
FOR BIT with the library's.  B(n) and the row caps are restated here independently of csrc/batch_plan.hpp."""
from collections import namedtuple

import numpy as np

from _ilu_ref import Scalar

OK, INSUFFICIENT_ITER, BREAKDOWN, INVALID_PRECOND = 0, 3, 4, 5

Result = namedtuple("Result", "status its res x")

WAVE = 64
VECTORS = {"cg": 5, "bicgstab": 8}          # x r z p q / x r r0 y p v t z
SCRATCH = 128                               # two rows of four 16-byte cells
BUDGET = 64 * 1024


def threads(n):
    """B(n) = min(256, 64 ceil(n / 64)), 64 for n = 0."""
    return 64 if n <= 0 else min(256, 64 * ((n + 63) // 64))


def max_rows(solver, dtype):
    """floor(64 KiB / (NV sizeof(T))) rounded down to a multiple of 64."""
    return BUDGET // (VECTORS[solver] * np.dtype(dtype).itemsize) // 64 * 64


def lds_bytes(solver, dtype, n):
    return SCRATCH + VECTORS[solver] * np.dtype(dtype).itemsize * n


class _Sys:
    """One system: the pattern as padded rows (entry e of every row that has one), its values in the real precision, and the
    operations of the statement on vectors."""

    def __init__(self, indptr, indices, data, nthreads=None):
        self.S = S = Scalar(data.dtype)
        self.T, self.R = S.T, np.dtype(S.R)
        self.n = n = indptr.size - 1
        self.B = threads(n) if nthreads is None else int(nthreads)
        ip = np.asarray(indptr, dtype=np.int64)
        ix = np.asarray(indices, dtype=np.int64)
        self.len = np.diff(ip)
        self.rows_e, self.col_e, self.val_e = [], [], []
        for e in range(int(self.len.max()) if n else 0):
            rows = np.nonzero(self.len > e)[0]
            self.rows_e.append(rows)
            self.col_e.append(ix[ip[rows] + e])
            self.val_e.append(self.vec(np.asarray(data)[ip[rows] + e]))
        rows = np.repeat(np.arange(n), self.len)
        d = np.full(n, -1, np.int64)
        d[rows[rows == ix]] = np.nonzero(rows == ix)[0]
        self.diag_pos = d
        self.data = np.asarray(data)
        self.eps = S.R(np.finfo(self.R).eps)

    # ---- vectors: a real array, or a (re, im) pair of them
    def vec(self, a):
        a = np.asarray(a, dtype=self.T)
        return (a.real.astype(self.R), a.imag.astype(self.R)) if self.S.cx else a.astype(self.R)

    def out(self, v):
        if self.S.cx:
            o = np.empty(v[0].shape, self.T)
            o.real = v[0]; o.imag = v[1]
            return o
        return np.array(v, dtype=self.T)

    def take(self, v, idx):
        return (v[0][idx], v[1][idx]) if self.S.cx else v[idx]

    def zeros(self, m):
        return (np.zeros(m, self.R), np.zeros(m, self.R)) if self.S.cx else np.zeros(m, self.R)

    def copy(self, v):
        return (v[0].copy(), v[1].copy()) if self.S.cx else v.copy()

    def put(self, v, idx, w):
        if self.S.cx:
            v[0][idx] = w[0]; v[1][idx] = w[1]
        else:
            v[idx] = w

    def conj(self, v):
        return (v[0], -v[1]) if self.S.cx else v

    def neg(self, s):
        return (-s[0], -s[1]) if self.S.cx else -s

    def one(self):
        r = self.S.R
        return (r(1.0), r(0.0)) if self.S.cx else r(1.0)

    def fromr(self, r):
        return (r, self.S.R(0.0)) if self.S.cx else r

    def re(self, s):
        return s[0] if self.S.cx else s

    def abs(self, s):
        return self.R.type(np.hypot(s[0], s[1])) if self.S.cx else self.R.type(abs(s))

    def sq(self, v):
        return v[0] * v[0] + v[1] * v[1] if self.S.cx else v * v

    def scal(self, s):
        """A scalar of Scalar's kind (f64: Python floats) as numpy scalars of the real precision: no operation below promotes."""
        r = self.S.R
        return (r(s[0]), r(s[1])) if self.S.cx else r(s)

    def div(self, a, b):
        with np.errstate(all="ignore"):
            if not self.S.cx:
                return self.S.R(a) / self.S.R(b)
            n = b[0] * b[0] + b[1] * b[1]
            return ((a[0] * b[0] + a[1] * b[1]) / n, (a[1] * b[0] - a[0] * b[1]) / n)

    # ---- the statement's operations
    def matvec(self, x):
        """The row fold, every row at once: entry e of the rows that have one, e ascending."""
        S = self.S
        y = self.zeros(self.n)
        for rows, col, val in zip(self.rows_e, self.col_e, self.val_e):
            self.put(y, rows, S.add(self.take(y, rows), S.mul(val, self.take(x, col))))
        return y

    def _tree(self, terms):
        """sum of a real array of n terms in the order of the statement."""
        B, n = self.B, terms.size
        k = (n + B - 1) // B
        pad = np.zeros(k * B, self.R)
        pad[:n] = terms
        part = np.zeros(B, self.R)                # thread t: from +0 over i = t, t + B, ..  (a padded +0 changes no partial: it is
        for j in range(k):                        # never -0 once +0 has been added to)
            part = part + pad[j * B:(j + 1) * B]
        q = part.reshape(B // WAVE, WAVE).copy()
        off = 32
        while off:
            q[:, :off] = q[:, :off] + q[:, off:2 * off]
            off >>= 1
        acc = q[0, 0]
        for w in range(1, B // WAVE):
            acc = acc + q[w, 0]
        return acc

    def sum(self, v):
        return (self._tree(v[0]), self._tree(v[1])) if self.S.cx else self._tree(v)

    def cdot(self, a, b):
        return self.sum(self.S.mul(self.conj(a), b))

    def norm2(self, a):
        return np.sqrt(self._tree(self.sq(a)))

    def dinv(self):
        """one / a_ii in T."""
        d = self.vec(self.data[self.diag_pos])
        one = (np.ones(self.n, self.R), np.zeros(self.n, self.R)) if self.S.cx else np.ones(self.n, self.R)
        return self.div(one, d)


def mul_vec(indptr, indices, values, X, nthreads=None):
    """Y_b = A_b X_b with the statement's row fold; values (nbatch, nnz), X (nbatch, n)."""
    Y = np.zeros_like(X)
    for b in range(values.shape[0]):
        A = _Sys(indptr, indices, values[b], nthreads)
        Y[b] = A.out(A.matvec(A.vec(X[b])))
    return Y


def bicgstab(indptr, indices, data, rhs, x0, max_iter, tol, jacobi=False, nthreads=None):
    """sprs_batch_bicgstab_solve_* for one system -> Result (res as the library reports it)."""
    A = _Sys(indptr, indices, data, nthreads)
    S, eps = A.S, A.eps
    R = S.R
    ax = lambda y, a, x: S.add(y, S.mul(x, a))            # y + x * a
    one, mone = A.one(), A.neg(A.one())
    rhs = A.vec(rhs); x = A.vec(x0)
    dinv = A.dinv() if jacobi else None
    with np.errstate(all="ignore"):
        rhs_norm = A.norm2(rhs)
        if rhs_norm <= eps:
            return Result(OK, 0, rhs_norm, A.out(A.zeros(A.n)))
        tol2 = R(tol) * rhs_norm
        r = ax(A.matvec(x), mone, rhs)
        r0 = A.copy(r)
        r0_norm = A.norm2(r0)
        if r0_norm <= tol2:
            return Result(OK, 0, r0_norm / rhs_norm, A.out(x))
        r0_norm_tol = r0_norm * eps
        r0_norm_tol = r0_norm_tol * r0_norm_tol
        rho = A.fromr(r0_norm * r0_norm)
        p = None
        if jacobi:
            p = A.copy(r)
            y = S.mul(p, dinv)
        else:
            y = A.copy(r)
        v = A.matvec(y)
        alpha = A.div(rho, A.cdot(r0, v))

        def half(x, r, alpha):
            na = A.neg(alpha)
            r = ax(r, na, v)
            sz = S.mul(r, dinv) if jacobi else r
            t = A.matvec(sz)
            tt = A.cdot(t, t)
            w = A.div(A.cdot(t, r), tt) if A.re(tt) > 0 else A.scal(S.zero())
            nw = A.neg(w)
            x = ax(x, na, y)
            x = ax(x, nw, sz)
            r = ax(r, nw, t)
            return x, r, w

        x, r, w = half(x, r, alpha)
        for its in range(1, int(max_iter)):
            r_norm = A.norm2(r)
            if r_norm <= tol2:
                return Result(OK, its, r_norm / rhs_norm, A.out(x))
            rho_old = rho
            rho = A.cdot(r0, r)
            if A.abs(rho) < r0_norm_tol:
                r = ax(A.matvec(x), mone, rhs)
                r0 = A.copy(r)
                rn = A.norm2(r)
                rho = A.fromr(rn * rn)
                r0_norm_tol = A.re(rho) * eps * eps
            beta = S.mul(A.div(rho, rho_old), A.div(alpha, w))
            c1 = S.mul(A.neg(beta), w)
            yp = p if jacobi else y
            yp = S.add(S.mul(v, c1), S.mul(yp, beta))
            yp = ax(yp, one, r)
            if jacobi:
                p = yp
                y = S.mul(p, dinv)
            else:
                y = yp
            v = A.matvec(y)
            tmp = A.cdot(r0, v)
            if A.abs(tmp) <= 0:
                return Result(BREAKDOWN, its, R(0.0), A.out(x))
            alpha = A.div(rho, tmp)
            x, r, w = half(x, r, alpha)
        return Result(INSUFFICIENT_ITER, int(max_iter), R(0.0), A.out(x))


def cg(indptr, indices, data, rhs, x0, max_iter, tol, jacobi=False, nthreads=None):
    """sprs_batch_cg_solve_* for one system -> Result."""
    A = _Sys(indptr, indices, data, nthreads)
    S, eps = A.S, A.eps
    R = S.R
    one, mone = A.one(), A.neg(A.one())
    rhs = A.vec(rhs); x = A.vec(x0)
    dinv = A.dinv() if jacobi else None
    with np.errstate(all="ignore"):
        rhs_norm = A.norm2(rhs)
        if rhs_norm <= eps:
            return Result(OK, 0, rhs_norm, A.out(A.zeros(A.n)))
        tol2 = R(tol) * rhs_norm
        r = S.add(S.mul(rhs, one), S.mul(A.matvec(x), mone))
        r_norm = A.norm2(r)
        if r_norm <= tol2:
            return Result(OK, 0, r_norm / rhs_norm, A.out(x))
        z = S.mul(r, dinv) if jacobi else r
        p = A.copy(z)
        rho = A.cdot(r, z)
        for its in range(int(max_iter)):
            q = A.matvec(p)
            pq = A.cdot(p, q)
            if not (A.re(pq) > 0):
                return Result(BREAKDOWN, its, R(0.0), A.out(x))
            alpha = A.div(rho, pq)
            x = S.add(x, S.mul(p, alpha))
            r = S.add(r, S.mul(q, A.neg(alpha)))
            r_norm = A.norm2(r)
            if r_norm <= tol2:
                return Result(OK, its + 1, r_norm / rhs_norm, A.out(x))
            z = S.mul(r, dinv) if jacobi else r
            rho_new = A.cdot(r, z)
            if jacobi and not (A.re(rho_new) > 0):
                return Result(INVALID_PRECOND, its, A.re(rho_new), A.out(x))
            beta = A.div(rho_new, rho)
            rho = rho_new
            p = S.add(S.mul(z, one), S.mul(p, beta))
        return Result(INSUFFICIENT_ITER, int(max_iter), R(0.0), A.out(x))


def solve_batch(solver, indptr, indices, values, rhs, x0, max_iter, tol, jacobi=False):
    """Every system of a batch -> (X, its, res, status) as the library's entry point fills them, and its return value."""
    fn = {"bicgstab": bicgstab, "cg": cg}[solver]
    nb = values.shape[0]
    T = np.dtype(values.dtype)
    X = np.array(x0, dtype=T)
    its = np.zeros(nb, np.int64); res = np.zeros(nb, Scalar(T).R); status = np.zeros(nb, np.int32)
    for b in range(nb):
        o = fn(indptr, indices, values[b], rhs[b], x0[b], max_iter, tol, jacobi)
        X[b] = o.x; its[b] = o.its; res[b] = o.res; status[b] = o.status
    ret = next((int(s) for s in status if s != OK), OK)
    return X, its, res, status, ret
