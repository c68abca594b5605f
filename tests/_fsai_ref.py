"""FSAI as include/sprsolve_hip.h states it (sprs_fsai_*), restated with plain loops in the scalar type under test: the checker of
tests/test_fsai_cpu.py and tests/test_gpu_fsai.py.  Every scalar operation rounds once in the type's precision; complex numbers
are (re, im) pairs worked component by component (tests/_ilu_ref.py's Scalar), so the rows of G can be compared BIT FOR BIT with
the library's.  `Applier` folds the rows of G and then the rows of GH left to right from zero (tests/_amg_ref.py's spmv, one
rounded operation per array operation), GH built as sprs_csr_adjoint states it: the bits of the two SpMVs."""
import math
from collections import namedtuple

import numpy as np

from _amg_ref import Ops, spmv
from _ilu_ref import Scalar

OK, INVALID_PRECOND, INVALID_ARGUMENT, ZERO_DIAGONAL = 0, 5, 7, 8
MAX_ROW = 64

Factor = namedtuple("Factor", "status row ip ix val")        # row: the offending row, else -1; ip / ix / val: G, None unless OK


class _S(Scalar):
    def rsqrt_arg(self, d):
        return np.sqrt(np.float32(d)) if self.single else math.sqrt(d)

    def re(self, a):
        return a[0] if self.cx else a

    def from_real(self, r):
        return (r, self._r(0.0)) if self.cx else r

    def sq(self, a):
        return a[0] * a[0] + a[1] * a[1] if self.cx else a * a

    def conj(self, a):
        return (a[0], -a[1]) if self.cx else a

    def neg(self, a):
        return (-a[0], -a[1]) if self.cx else -a

    def divr(self, a, r):
        return (self._div(a[0], r), self._div(a[1], r)) if self.cx else self._div(a, r)


def pattern(indptr, indices, power):
    """-> per row the ascending columns j <= i of pattern(A) (power 1) or of the structural pattern of A A (power 2)."""
    n = indptr.size - 1
    rows = [indices[indptr[i]:indptr[i + 1]].astype(np.int64) for i in range(n)]
    out = []
    for i in range(n):
        c = rows[i] if power == 1 else (np.unique(np.concatenate([rows[k] for k in rows[i]])) if rows[i].size else rows[i])
        out.append(c[c <= i])
    return out


def row_of_g(S, J, arow):
    """Steps 2 to 4 for one row: J ascending, arow(j) -> {column: scalar} of row j of A.  -> (OK, [g_p]) or (INVALID_PRECOND, None)."""
    m = len(J)
    c = [[None] * (p + 1) for p in range(m)]
    for p in range(m):
        r = arow(J[p])
        for q in range(p + 1):
            v = r.get(J[q])
            c[p][q] = S.zero() if v is None else (S.from_real(S.re(v)) if q == p else v)
    for q in range(m):
        d = S.re(c[q][q])
        for k in range(q):
            d = d - S.sq(c[q][k])
        if not (np.isfinite(d) and d > 0):
            return INVALID_PRECOND, None
        cqq = S.rsqrt_arg(d)
        for p in range(q + 1, m):
            t = c[p][q]
            for k in range(q):
                t = S.sub(t, S.mul(c[p][k], S.conj(c[q][k])))
            c[p][q] = S.divr(t, cqq)
        c[q][q] = S.from_real(cqq)
    g = [None] * m
    g[m - 1] = S.from_real(S._div(S._r(1.0), S.re(c[m - 1][m - 1])))
    for p in range(m - 2, -1, -1):
        acc = S.zero()
        for q in range(m - 1, p, -1):
            acc = S.add(acc, S.mul(c[q][p], g[q]))
        g[p] = S.divr(S.neg(acc), S.re(c[p][p]))
    return OK, g


def fsai(indptr, indices, data, power=1, rows=None):
    """-> Factor.  rows: compute the values of these rows only (the others stay zero): a spot check of a large matrix."""
    n = indptr.size - 1
    for i in range(n):
        if np.any(np.diff(indices[indptr[i]:indptr[i + 1]]) <= 0):
            return Factor(INVALID_ARGUMENT, i, None, None, None)
    Js = pattern(indptr, indices, power)
    for i in range(n):
        if Js[i].size == 0 or Js[i][-1] != i or i not in indices[indptr[i]:indptr[i + 1]]:
            return Factor(ZERO_DIAGONAL, i, None, None, None)
    for i in range(n):
        if Js[i].size > MAX_ROW:
            return Factor(INVALID_ARGUMENT, i, None, None, None)
    S = _S(data.dtype)
    cache = {}

    def arow(j):
        if j not in cache:
            cache[j] = {int(indices[k]): S.load(data[k]) for k in range(indptr[j], indptr[j + 1]) if indices[k] <= j}
        return cache[j]

    gp = np.zeros(n + 1, np.int32); np.cumsum([J.size for J in Js], out=gp[1:])
    gx = np.concatenate(Js).astype(np.int32) if n else np.zeros(0, np.int32)
    gv = np.zeros(gx.size, data.dtype)
    for i in (range(n) if rows is None else rows):
        st, g = row_of_g(S, [int(j) for j in Js[i]], arow)
        if st != OK:
            return Factor(st, i, None, None, None)
        gv[gp[i]:gp[i + 1]] = S.vec_store(g)
        if rows is None and len(cache) > 4096:
            cache.clear()
    return Factor(OK, -1, gp, gx, gv)


def adjoint(gp, gx, gv):
    """GH as sprs_csr_adjoint(G, 1) builds it: row j holds column j's entries in ascending original row, conjugated."""
    n = gp.size - 1
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(gp))
    order = np.argsort(gx, kind="stable")
    hp = np.zeros(n + 1, np.int32); np.cumsum(np.bincount(gx, minlength=n), out=hp[1:])
    return hp, rows[order], Ops(gv.dtype).conj(gv[order]).astype(gv.dtype)


class Applier:
    """v -> GH (G v) with the bits of two row folds."""

    def __init__(self, gp, gx, gv):
        self.op = Ops(gv.dtype)
        self.G = (gp, gx, gv)
        self.GH = adjoint(gp, gx, gv)

    def __call__(self, v):
        v = np.asarray(v, dtype=self.op.T)
        return spmv(self.op, *self.GH, spmv(self.op, *self.G, v))


def dense(ip, ix, val, n=None):
    n = ip.size - 1 if n is None else n
    M = np.zeros((ip.size - 1, n), val.dtype)
    M[np.repeat(np.arange(ip.size - 1), np.diff(ip)), ix] = val
    return M
