"""Smoothed-aggregation AMG as include/sprsolve_hip.h states it (sprs_amg_*): the checker of tests/test_amg_cpu.py and
tests/test_gpu_amg.py.  The rules that decide something (strength, the three aggregation passes, the stopping tests) are plain
Python loops over the rows.  The arithmetic is numpy's, one separately rounded operation of the scalar type per array operation
(complex numbers by components with csrc/scalar.hpp's naive formulas), and every sum is folded in the order the header states:
`_fold` adds the t-th term of every segment in step t, so a segment's value has the bits of the serial left-to-right loop.  That
keeps the 32 768-row cases of the GPU file to a second or two where scalar loops would take minutes."""
from collections import namedtuple

import numpy as np

OK, DIM_MISMATCH, INVALID_ARGUMENT, ZERO_DIAGONAL, NOT_SQUARE = 0, 6, 7, 8, 9
COARSE_SWEEPS = 8            # damped-Jacobi sweeps that stand for the coarse solve when the coarsest level is too large for the LU
COARSE_LIMIT = 1024          # largest coarse_max (the dense LU is applied by one workgroup)
LEVELS_LIMIT = 32            # largest max_levels

Level = namedtuple("Level", "n ip ix val diag omega agg P R")      # agg / P / R: None on the coarsest level; P, R: (ip, ix, val)
Hierarchy = namedtuple("Hierarchy", "status row levels lu dtype")  # lu: dense LU of the coarsest level, or None (Jacobi sweeps)


class Ops:
    """Element-wise scalar operations of dtype T on numpy arrays, each real operation rounded once."""

    def __init__(self, dtype):
        self.T = np.dtype(dtype)
        self.cx = self.T.kind == "c"
        self.R = np.dtype(np.float32 if self.T in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)

    def make(self, re, im):
        out = np.empty(np.broadcast(re, im).shape, self.T)
        out.real = re; out.imag = im
        return out

    def add(self, a, b):
        return self.make(a.real + b.real, a.imag + b.imag) if self.cx else a + b

    def sub(self, a, b):
        return self.make(a.real - b.real, a.imag - b.imag) if self.cx else a - b

    def mul(self, a, b):
        if not self.cx:
            return a * b
        return self.make(a.real * b.real - a.imag * b.imag, a.real * b.imag + a.imag * b.real)

    def mulr(self, a, r):
        return self.make(a.real * r, a.imag * r) if self.cx else a * r

    def div(self, a, b):
        with np.errstate(all="ignore"):
            if not self.cx:
                return a / b
            n = b.real * b.real + b.imag * b.imag
            return self.make((a.real * b.real + a.imag * b.imag) / n, (a.imag * b.real - a.real * b.imag) / n)

    def conj(self, a):
        return self.make(a.real, -a.imag) if self.cx else a

    def sq(self, a):
        """|a|^2"""
        return a.real * a.real + a.imag * a.imag if self.cx else a * a

    def mod(self, a):
        """|a|: fabs, or sqrt(re re + im im) (not hypot: every step is one IEEE operation)"""
        return np.sqrt(self.sq(a)) if self.cx else np.abs(a)

    def bad_pivot(self, a):
        return ~(np.isfinite(a.real) & np.isfinite(a.imag)) | ((a.real == 0) & (a.imag == 0))


def _fold(op, seg_start, seg_len, terms):
    """acc_s = (((0 + terms[start_s]) + terms[start_s + 1]) + ...) for every segment s."""
    acc = np.zeros(seg_start.size, op.T)
    for t in range(int(seg_len.max()) if seg_len.size else 0):
        sel = np.nonzero(seg_len > t)[0]
        acc[sel] = op.add(acc[sel], terms[seg_start[sel] + t])
    return acc


def spmv(op, ip, ix, val, x):
    """sigma_i = sum_j a_ij x_j folded left to right from zero."""
    return _fold(op, ip[:-1], np.diff(ip), op.mul(val, x[ix]))


def spgemm(op, ncols, aip, aix, av, bip, bix, bv):
    """C = A B row by row in Gustavson order (for a_ik with k ascending, for b_kj with j ascending: acc_j += a_ik b_kj, acc from
    zero); the stored pattern is the structural one, columns ascending."""
    n = aip.size - 1
    cnt = np.diff(bip)[aix]
    off = np.concatenate([[0], np.cumsum(cnt)])
    a_idx = np.repeat(np.arange(aix.size), cnt)
    b_idx = bip[aix][a_idx] + (np.arange(off[-1]) - off[a_idx])
    rows = np.repeat(np.repeat(np.arange(n), np.diff(aip)), cnt)
    cols = bix[b_idx].astype(np.int64)
    prod = op.mul(av[a_idx], bv[b_idx])
    order = np.lexsort((cols, rows))                         # stable: equal (row, col) keep their generation order
    key = rows[order] * ncols + cols[order]
    first = np.concatenate([[True], key[1:] != key[:-1]]) if key.size else np.zeros(0, bool)
    start = np.nonzero(first)[0]
    seglen = np.diff(np.concatenate([start, [key.size]]))
    val = _fold(op, start, seglen, prod[order])
    crow, ccol = rows[order][start], cols[order][start]
    cip = np.zeros(n + 1, np.int64); np.cumsum(np.bincount(crow, minlength=n), out=cip[1:])
    return cip, ccol, val


def transpose_conj(op, ncols, ip, ix, val):
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    order = np.lexsort((rows, ix))
    tip = np.zeros(ncols + 1, np.int64); np.cumsum(np.bincount(ix, minlength=ncols), out=tip[1:])
    return tip, rows[order], op.conj(val[order])


def aggregate(op, ip, ix, val, diag, theta, passes=3):
    """The three passes -> (agg, count).  j != i is strong for row i when |a_ij|^2 >= (theta theta) (|a_ii| |a_jj|).
    passes=2 stops before pass 3 (rows it would have placed keep -1): tests/test_amg_cpu.py shows that there are none."""
    n = ip.size - 1
    R = op.R.type
    rows = np.repeat(np.arange(n), np.diff(ip))
    md = op.mod(diag)
    sq = op.sq(val)
    th2 = R(theta) * R(theta)
    strong = (ix != rows) & (sq >= th2 * (md[rows] * md[ix]))
    ipl = [int(v) for v in ip]; ixl = [int(v) for v in ix]; stl = strong.tolist(); sql = sq.tolist()
    agg = [-1] * n
    count = 0
    for i in range(n):                                       # pass 1
        if agg[i] >= 0:
            continue
        nb = [ixl[p] for p in range(ipl[i], ipl[i + 1]) if stl[p]]
        if all(agg[j] < 0 for j in nb):
            agg[i] = count
            for j in nb:
                agg[j] = count
            count += 1
    snap = list(agg)
    for i in range(n):                                       # pass 2
        if snap[i] >= 0:
            continue
        best, bj = -1.0, -1
        for p in range(ipl[i], ipl[i + 1]):
            if stl[p] and snap[ixl[p]] >= 0 and sql[p] > best:
                best, bj = sql[p], ixl[p]
        if bj >= 0:
            agg[i] = snap[bj]
    for i in range(n if passes >= 3 else 0):                 # pass 3
        if agg[i] >= 0:
            continue
        agg[i] = count
        for p in range(ipl[i], ipl[i + 1]):
            if stl[p] and agg[ixl[p]] < 0:
                agg[ixl[p]] = count
        count += 1
    return np.array(agg, np.int64), count


def _omega(op, ip, val, diag):
    """omega = 4 / (3 rho), rho = max_i (sum_j |a_ij|, folded left to right from zero) / |a_ii|."""
    R = op.R.type
    rowsum = _fold(Ops(op.R), ip[:-1], np.diff(ip), op.mod(val))
    rho = np.max(rowsum / op.mod(diag)) if diag.size else R(1)
    return R(4) / (R(3) * rho)


def dense_lu(op, M):
    """No-pivot LU in place, the k-i-j order -> (status, row, LU)."""
    a = M.copy()
    n = a.shape[0]
    for k in range(n):
        if op.bad_pivot(a[k, k]):
            return ZERO_DIAGONAL, k, None
        l = op.div(a[k + 1:, k], a[k, k])
        a[k + 1:, k] = l
        a[k + 1:, k + 1:] = op.sub(a[k + 1:, k + 1:], op.mul(l[:, None], a[k, k + 1:][None, :]))
    return OK, -1, a


def build(indptr, indices, data, theta=0.08, coarse_max=256, max_levels=16, ncols=None):
    """The hierarchy of the header -> Hierarchy."""
    op = Ops(data.dtype)
    n = indptr.size - 1
    if ncols is not None and ncols != n:
        return Hierarchy(NOT_SQUARE, -1, None, None, op.T)
    if not (theta >= 0) or coarse_max < 1 or coarse_max > COARSE_LIMIT or max_levels < 1 or max_levels > LEVELS_LIMIT:
        return Hierarchy(INVALID_ARGUMENT, -1, None, None, op.T)
    ip = np.asarray(indptr, np.int64); ix = np.asarray(indices, np.int64); val = np.asarray(data)
    for i in range(n):
        if np.any(np.diff(ix[ip[i]:ip[i + 1]]) <= 0):
            return Hierarchy(INVALID_ARGUMENT, i, None, None, op.T)
    levels = []
    lvl = 0
    while True:
        rows = np.repeat(np.arange(n), np.diff(ip))
        on = rows == ix
        bad = np.ones(n, bool)                               # no stored diagonal, or one that is zero or not finite
        bad[rows[on]] = op.bad_pivot(val[on])
        if bad.any():
            return Hierarchy(ZERO_DIAGONAL, int(np.nonzero(bad)[0][0]), None, None, op.T)
        diag = val[on]
        omega = _omega(op, ip, val, diag)
        if n <= coarse_max or lvl + 1 >= max_levels:
            break
        agg, nc = aggregate(op, ip, ix, val, diag, op.R.type(theta) * op.R.type(2.0 ** -lvl))
        if 2 * nc > n:                                       # the half-rows stop: this level is the coarsest
            break
        tip = np.arange(n + 1, dtype=np.int64)
        aip, aix, av = spgemm(op, nc, ip, ix, val, tip, agg, np.ones(n, op.T))          # A T
        arow = np.repeat(np.arange(n), np.diff(aip))
        t = (aix == agg[arow]).astype(op.T)
        pv = op.sub(t, op.div(op.mulr(av, omega), diag[arow]))                           # t_ic - (omega (A T)_ic) / d_i
        P = (aip, aix, pv)
        Rm = transpose_conj(op, nc, *P)
        apip, apix, apv = spgemm(op, nc, ip, ix, val, *P)
        cip, cix, cv = spgemm(op, nc, *Rm, apip, apix, apv)
        levels.append(Level(n, ip, ix, val, diag, omega, agg, P, Rm))
        ip, ix, val, n = cip, cix, cv, nc
        lvl += 1
    levels.append(Level(n, ip, ix, val, diag, omega, None, None, None))
    lu = None
    if n <= coarse_max:
        M = np.zeros((n, n), op.T); M[np.repeat(np.arange(n), np.diff(ip)), ix] = val
        st, row, lu = dense_lu(op, M)
        if st != OK:
            return Hierarchy(st, row, None, None, op.T)
    return Hierarchy(OK, -1, levels, lu, op.T)


class Applier:
    """One V(1,1) cycle on a Hierarchy: callable v -> M v, the preconditioner of ref.cg / ref.gmres."""

    def __init__(self, H):
        assert H.status == OK
        self.H = H
        self.op = Ops(H.dtype)

    def _jacobi(self, L, b, x):
        op = self.op
        return op.add(x, op.div(op.mulr(op.sub(b, spmv(op, L.ip, L.ix, L.val, x)), L.omega), L.diag))

    def _coarse(self, L, b):
        op = self.op
        if self.H.lu is None:
            x = op.div(op.mulr(b, L.omega), L.diag)
            for _ in range(COARSE_SWEEPS - 1):
                x = self._jacobi(L, b, x)
            return x
        lu = self.H.lu
        w = b.copy()
        n = w.size
        for j in range(n):                                   # w_i = ((b_i - l_i0 w_0) - l_i1 w_1) - ...
            w[j + 1:] = op.sub(w[j + 1:], op.mul(lu[j + 1:, j], w[j]))
        for j in range(n - 1, -1, -1):                       # x_j = (((w_j - u_j,n-1 x_n-1) - ...) - u_j,j+1 x_j+1) / u_jj
            w[j] = op.div(w[j], lu[j, j])
            w[:j] = op.sub(w[:j], op.mul(lu[:j, j], w[j]))
        return w

    def cycle(self, l, b):
        op = self.op
        L = self.H.levels[l]
        if l == len(self.H.levels) - 1:
            return self._coarse(L, b)
        x = op.div(op.mulr(b, L.omega), L.diag)              # pre-smoothing from zero
        r = op.sub(b, spmv(op, L.ip, L.ix, L.val, x))
        bc = spmv(op, *L.R, r)
        ec = self.cycle(l + 1, bc)
        x = op.add(x, spmv(op, *L.P, ec))
        return self._jacobi(L, b, x)

    def __call__(self, v):
        return self.cycle(0, np.asarray(v, dtype=self.H.dtype))
