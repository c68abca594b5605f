"""The LOBPCG recurrence of include/sprsolve_hip.h (sprs_lobpcg_*) restated in numpy: vectors, residuals and the Gram sums in
the dtype under test, the projected problem (scaling, Cholesky, the Hermitian Jacobi eigensolver, the coefficient block) in
double or complex double.  It is the checker of tests/test_lobpcg_cpu.py and tests/test_gpu_lobpcg.py.  The sums associate
differently from the library's, so nothing is compared bit for bit against it and its iteration counts only cap the library's."""
from collections import namedtuple

import numpy as np

from _eigsh_ref import (BREAKDOWN, EPS64, INSUFFICIENT_ITER, LARGEST, MAX_SWEEPS, OK, SMALLEST, _matvec, default_tol, dense, order, pairs,  # noqa: F401
                        real_dtype)

MAX_BLOCK = 8

Result = namedtuple("Result", "status vals X res nconv iters restarts matvecs sweeps")
RR = namedtuple("RR", "ok theta C sweeps used_p fell_back anorm")


def default_block(n):
    return min(MAX_BLOCK, n // 6)


def block_ok(b, n):
    """The rule of create: 1 <= b <= 8 and 6 b <= n."""
    return 1 <= b <= MAX_BLOCK and 6 * b <= n


def default_X0(n, b, dt):
    """What Lobpcg.solve(X0=None) uses: column c is stream 100 + 2 c (+ 1j stream 101 + 2 c)."""
    from sprsolve_amd import gen
    X = np.zeros((b, n), dt)
    for c in range(b):
        v = gen.uniform(gen.SEED, n, stream=100 + 2 * c)
        if np.dtype(dt).kind == "c":
            v = v + 1j * gen.uniform(gen.SEED, n, stream=101 + 2 * c)
        X[c] = v.astype(dt)
    return X


def jacobi_eigh_h(K):
    """-> (theta, Z, sweeps, converged): K = Z diag(theta) Z^H, unsorted, by cyclic Jacobi on a Hermitian K (real or complex) in
    double: _eigsh_ref.jacobi_eigh's order and stopping rule, the rotation carrying the phase u = K_pq / |K_pq| of its pivot:
    x_p' = c x_p - conj(s u) x_q, x_q' = (s u) x_p + c x_q on the columns of K and Z, row_p' = c row_p - (s u) row_q,
    row_q' = conj(s u) row_p + c row_q on K's rows, then K_pq = K_qp = 0 and Im K_pp = Im K_qq = 0 exactly."""
    K = np.asarray(K)
    cd = np.complex128 if K.dtype.kind == "c" else np.float64
    me = K.shape[0]
    M = (me + 1) & ~1
    A = np.zeros((M, M), cd); A[:me, :me] = K
    Z = np.eye(M, dtype=cd)
    with np.errstate(all="ignore"):
        fro2 = float(np.sum(np.abs(A) ** 2))
    sweeps, conv = 0, False
    if not np.isfinite(fro2):
        return np.real(np.diag(A))[:me].copy(), Z[:me, :me].copy(), MAX_SWEEPS, False
    while True:
        B = A.copy(); np.fill_diagonal(B, 0.0)
        off2 = float(np.sum(np.abs(B) ** 2))
        if off2 <= EPS64 * EPS64 * fro2:
            conv = True
            break
        if sweeps == MAX_SWEEPS:
            break
        for r in range(M - 1):
            p, q = pairs(r, M)
            apq = A[p, q]
            mag = np.abs(apq)
            nz = mag != 0.0
            with np.errstate(all="ignore"):
                u = np.where(nz, apq / np.where(nz, mag, 1.0), 1.0)
                tau = (A[q, q].real - A[p, p].real) / (2.0 * np.where(nz, mag, 1.0))
                t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
            c = np.where(nz, c, 1.0); sc = np.where(nz, s * u, 0.0)
            for Xm in (A, Z):
                xp, xq = Xm[:, p].copy(), Xm[:, q].copy()
                Xm[:, p] = c * xp - np.conj(sc) * xq; Xm[:, q] = sc * xp + c * xq
            xp, xq = A[p, :].copy(), A[q, :].copy()
            A[p, :] = c[:, None] * xp - sc[:, None] * xq; A[q, :] = np.conj(sc)[:, None] * xp + c[:, None] * xq
            A[p, q] = 0.0; A[q, p] = 0.0
            A[p, p] = A[p, p].real; A[q, q] = A[q, q].real
        sweeps += 1
    return np.real(np.diag(A))[:me].copy(), Z[:me, :me].copy(), sweeps, conv


def _project(G, K, epsR):
    """Steps (2) - (6) and (8) on one index set: -> (theta, C, sweeps) or None on a failure of the scaling or the Cholesky rule.
    A Jacobi that does not converge returns theta = None."""
    m = G.shape[0]
    d = np.real(np.diag(G))
    if not np.all(d > 0.0):
        return None
    s = 1.0 / np.sqrt(d)
    Gh = s[:, None] * G * s[None, :]
    L = np.zeros_like(Gh)
    for j in range(m):
        with np.errstate(all="ignore"):
            piv = float(np.real(Gh[j, j]) - np.sum(np.abs(L[j, :j]) ** 2))
        if not piv > 64.0 * m * epsR:
            return None
        L[j, j] = np.sqrt(piv)
        for i in range(j + 1, m):
            L[i, j] = (np.conj(Gh[j, i]) - np.sum(L[i, :j] * np.conj(L[j, :j]))) / L[j, j]     # Gh_ij from the upper triangle
    Ks = s[:, None] * K * s[None, :]
    import scipy.linalg as sl
    with np.errstate(all="ignore"):
        M1 = sl.solve_triangular(L, Ks, lower=True, check_finite=False)
        Kh = sl.solve_triangular(L, M1.conj().T, lower=True, check_finite=False).conj().T
    Kh = np.triu(Kh) + np.triu(Kh, 1).conj().T
    Kh[np.arange(m), np.arange(m)] = np.real(np.diag(Kh))
    theta, Z, sweeps, conv = jacobi_eigh_h(Kh)
    if not conv:
        return (None, None, sweeps)
    with np.errstate(all="ignore"):
        C = s[:, None] * sl.solve_triangular(L.conj().T, Z, lower=False, check_finite=False)
    return theta, C, sweeps


def herm_from_upper(M):
    """The matrix the projected problem takes for K (and G): the upper triangle, its conjugate below, a real diagonal."""
    H = np.triu(M) + np.triu(M, 1).conj().T
    H[np.arange(M.shape[0]), np.arange(M.shape[0])] = np.real(np.diag(M))
    return H


def rayleigh_ritz(G, K, b, with_p, which, epsR, lock=None):
    """G, K: (3 b, 3 b) in the order [X, P, W] (the P rows and columns are ignored unless with_p; (b, b) for the start step).
    lock: b booleans, the soft-locked columns, whose P_c and W_c are left out of the problem (None: none is locked).
    -> RR: theta sorted for `which` (all of the problem's), C with 3 b rows (zero where a vector was left out) and the columns
    in theta's order, anorm = the largest |K_ii| / G_ii over the X and W columns of the problem solved."""
    m3 = G.shape[0]
    G = herm_from_upper(np.asarray(G)); K = herm_from_upper(np.asarray(K))
    tries = []
    if m3 == b:
        tries.append(np.arange(b))
    else:
        free = np.arange(b) if lock is None else np.flatnonzero(~np.asarray(lock, bool))
        if with_p:
            tries.append(np.concatenate([np.arange(b), b + free, 2 * b + free]))
        tries.append(np.concatenate([np.arange(b), 2 * b + free]))
    fell = False
    for t, idx in enumerate(tries):
        out = _project(G[np.ix_(idx, idx)], K[np.ix_(idx, idx)], epsR)
        if out is None:
            fell = fell or (with_p and t == 0 and len(tries) == 2)
            continue
        theta, Cs, sweeps = out
        if theta is None:
            return RR(False, None, None, sweeps, False, fell, 0.0)
        o = order(theta, which)
        C = np.zeros((m3, idx.size), Cs.dtype)
        C[idx] = Cs[:, o]
        xw = idx[(idx < b) | (idx >= 2 * b)]
        rq = float(np.max(np.abs(np.real(np.diag(K))[xw]) / np.real(np.diag(G))[xw]))
        return RR(True, theta[o], C, sweeps, with_p and t == 0 and m3 != b, fell, rq)
    return RR(False, None, None, 0, False, fell, 0.0)


def lobpcg(indptr, indices, data, k, which, X0, max_iter, tol, prec=None):
    """-> Result.  X0: (b, n) in data's dtype.  prec: None, a real or complex array (the diagonal of M) or a callable r -> M r.
    X has shape (k, n) (None on BREAKDOWN)."""
    T_ = np.dtype(data.dtype)
    R = real_dtype(T_)
    cd = np.complex128 if T_.kind == "c" else np.float64
    n = indptr.size - 1
    X0 = np.asarray(X0, T_)
    b = X0.shape[0]
    assert block_ok(b, n) and 1 <= k <= b and which in (LARGEST, SMALLEST) and max_iter >= 1 and X0.shape == (b, n)
    A = _matvec(indptr, indices, data)
    epsR = float(np.finfo(R).eps)
    zk = np.zeros(k)

    def gram(S, AS):
        with np.errstate(all="ignore"):
            return (S.conj() @ S.T).astype(cd), (S.conj() @ AS.T).astype(cd)

    def rotate(S, C):
        with np.errstate(all="ignore"):
            return np.ascontiguousarray((S.T @ C.astype(T_)).T.astype(T_))

    with np.errstate(all="ignore"):
        X = X0.copy()
        AX = np.stack([A(x) for x in X])
    matvecs, restarts, anorm, most = b, 0, 0.0, 0
    rr = rayleigh_ritz(*gram(X, AX), b, False, which, epsR)
    most = max(most, rr.sweeps)
    if not rr.ok:
        return Result(BREAKDOWN, zk, None, zk, 0, 0, 0, matvecs, most)
    anorm = max(anorm, rr.anorm)
    X, AX = rotate(X, rr.C), rotate(AX, rr.C)
    theta = rr.theta[:b].copy()
    P = np.zeros_like(X); AP = np.zeros_like(X)
    with_p = False
    it = 0
    while True:
        it += 1
        with np.errstate(all="ignore"):
            Rm = (AX - theta.astype(R)[:, None].astype(T_) * X).astype(T_)
            res = np.sqrt(np.sum((Rm.real * Rm.real + Rm.imag * Rm.imag).astype(R), axis=1, dtype=R)).astype(np.float64)
        if not np.all(np.isfinite(res)):
            return Result(BREAKDOWN, theta[:k], None, res[:k], 0, it - 1, restarts, matvecs, most)
        lock = res <= tol * anorm                    # soft locking: these columns' P_c and W_c stay out of the projected problem
        nconv = 0
        while nconv < k and lock[nconv]:
            nconv += 1
        if nconv == k or it > max_iter:
            return Result(OK if nconv == k else INSUFFICIENT_ITER, theta[:k].copy(), X[:k].copy(), res[:k].copy(), nconv, it - 1, restarts,
                          matvecs, most)
        with np.errstate(all="ignore"):
            if prec is None:
                W = Rm
            elif callable(prec):
                W = np.stack([np.asarray(prec(r), T_) for r in Rm])
            else:
                W = (Rm * np.asarray(prec)[None, :]).astype(T_)
            AW = np.stack([A(w) for w in W])
        matvecs += b
        S = np.concatenate([X, P, W]); AS = np.concatenate([AX, AP, AW])
        rr = rayleigh_ritz(*gram(S, AS), b, with_p, which, epsR, lock)
        most = max(most, rr.sweeps)
        restarts += 1 if rr.fell_back else 0
        if not rr.ok:
            return Result(BREAKDOWN, theta[:k], None, res[:k], nconv, it, restarts, matvecs, most)
        anorm = max(anorm, rr.anorm)
        CX = rr.C[:, :b]
        CP = CX.copy(); CP[:b] = 0.0
        X, P, AX, AP = rotate(S, CX), rotate(S, CP), rotate(AS, CX), rotate(AS, CP)
        theta = rr.theta[:b].copy()
        with_p = True
