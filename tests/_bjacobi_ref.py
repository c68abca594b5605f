"""Block-Jacobi as include/sprsolve_hip.h states it (sprs_bjacobi_*), restated with plain loops in the scalar type under test: the
checker of tests/test_bjacobi_cpu.py and tests/test_gpu_bjacobi.py.  Every scalar operation rounds once in the type's precision;
complex numbers are (re, im) pairs worked component by component (tests/_ilu_ref.py's Scalar), so the inverse blocks and the
application can be compared BIT FOR BIT with the library's."""
from collections import namedtuple

import numpy as np

from _gmres_ref import _matvec, _tree
from _ilu_ref import BREAKDOWN, INSUFFICIENT_ITER, CgResult, Scalar

OK, INVALID_PRECOND, INVALID_ARGUMENT = 0, 5, 7
MAX_BLOCK = 32

Inverse = namedtuple("Inverse", "status row block_ptr blocks")   # row: the offending row, else -1; blocks: [(m, m) array], None unless OK


class _S(Scalar):
    def one(self):
        return (self._r(1.0), self._r(0.0)) if self.cx else self._r(1.0)

    def mag(self, a):
        return abs(a[0]) + abs(a[1]) if self.cx else abs(a)


def block_ptr_of(n, block_size):
    return np.array(list(range(0, n, block_size)) + [n], np.int64)


def invert(S, W):
    """Gauss-Jordan on [W | I] with implicit row pivoting; W: m x m nested lists of scalars (consumed).  -> the inverse as nested
    lists, or None where a pivot is zero or not finite."""
    m = len(W)
    V = [[S.one() if i == j else S.zero() for j in range(m)] for i in range(m)]
    used = [False] * m
    perm = [0] * m
    for k in range(m):
        p, best = -1, None
        for i in range(m):
            if used[i]:
                continue
            g = S.mag(W[i][k])
            if p < 0 or g > best:
                p, best = i, g
        if not (best > 0 and np.isfinite(best)):
            return None
        used[p] = True; perm[k] = p
        piv = W[p][k]
        for j in range(m):
            W[p][j] = S.div(W[p][j], piv)
            V[p][j] = S.div(V[p][j], piv)
        for i in range(m):
            if i == p:
                continue
            f = W[i][k]
            for j in range(m):
                W[i][j] = S.sub(W[i][j], S.mul(f, W[p][j]))
                V[i][j] = S.sub(V[i][j], S.mul(f, V[p][j]))
    return [V[perm[k]] for k in range(m)]


def local_matrix(S, indptr, indices, data, s, e):
    W = [[S.zero() for _ in range(e - s)] for _ in range(e - s)]
    for i in range(s, e):
        for k in range(indptr[i], indptr[i + 1]):
            c = int(indices[k])
            if s <= c < e:
                W[i - s][c - s] = S.load(data[k])
    return W


def bjacobi(indptr, indices, data, block_size=None, block_ptr=None, blocks=None):
    """-> Inverse.  blocks: invert these blocks only (the others stay None): a spot check of a large matrix."""
    n = indptr.size - 1
    bp = block_ptr_of(n, block_size) if block_ptr is None else np.asarray(block_ptr, np.int64)
    for i in range(n):
        if np.any(np.diff(indices[indptr[i]:indptr[i + 1]]) <= 0):
            return Inverse(INVALID_ARGUMENT, i, bp, None)
    S = _S(data.dtype)
    out = [None] * (bp.size - 1)
    with np.errstate(all="ignore"):
        for b in (range(bp.size - 1) if blocks is None else blocks):
            s, e = int(bp[b]), int(bp[b + 1])
            X = invert(S, local_matrix(S, indptr, indices, data, s, e))
            if X is None:
                return Inverse(INVALID_PRECOND, s, bp, None)
            out[b] = np.array([[S.store(x) for x in row] for row in X], dtype=data.dtype).reshape(e - s, e - s)
    return Inverse(OK, -1, bp, out)


class Applier:
    """v -> blockdiag(X_b) v with the bits of the row fold: j ascending from +0, acc = acc + X[i][j] * v[s + j]."""

    def __init__(self, block_ptr, blocks):
        self.S = _S(blocks[0].dtype)
        self.bp = [int(v) for v in block_ptr]
        self.X = [[self.S.vec_load(row) for row in X] for X in blocks]
        self.dtype = blocks[0].dtype

    def __call__(self, v):
        S = self.S
        x = S.vec_load(np.asarray(v, dtype=self.dtype))
        out = [None] * len(x)
        with np.errstate(all="ignore"):
            for b, X in enumerate(self.X):
                s = self.bp[b]
                for i, row in enumerate(X):
                    acc = S.zero()
                    for j, a in enumerate(row):
                        acc = S.add(acc, S.mul(a, x[s + j]))
                    out[s + i] = acc
        return S.vec_store(out)


def cg(indptr, indices, data, rhs, x0, max_iter, tol, prec=None, sums="numpy"):
    """tests/_ilu_ref.py's cg, statement for statement, with that file's gmres's choice of sums: "numpy" (numpy's own summation, the
    bits of _ilu_ref.cg) or "pairwise" (_gmres_ref._tree).  The second is what derives the comparable part of a long run."""
    T = np.dtype(data.dtype)
    R = np.dtype(np.float32 if T in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    n = indptr.size - 1
    rhs = np.asarray(rhs, dtype=T); x = np.array(x0, dtype=T)
    A = _matvec(indptr, indices, data)
    one = T.type(1)
    if sums == "numpy":
        norm2 = lambda v: R.type(np.linalg.norm(v))
        cdot = lambda a, b: T.type(np.vdot(a, b))
    else:
        norm2 = lambda v: R.type(np.sqrt(_tree((v.real * v.real + v.imag * v.imag).astype(R))))
        cdot = lambda a, b: T.type(_tree((np.conj(a) * b).astype(T)))
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
