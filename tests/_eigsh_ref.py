"""The thick-restart Lanczos recurrence of include/sprsolve_hip.h (sprs_eigsh_*) restated in numpy, in the dtype under test
with the projected matrix T in float64: the checker of tests/test_eigsh_cpu.py and tests/test_gpu_eigsh.py.  The Jacobi
eigensolver follows the header's order (round-robin pairs, the rotated entry set to exactly zero).  Vector operations round once
per operation in the dtype under test as the library's do; the sums (dot products, norms, the rows of the matrix product and of
V S) associate differently, so nothing is compared bit for bit against it."""
from collections import namedtuple

import numpy as np

OK, INCOMPATIBLE_RHS_SIZE, INCOMPATIBLE_X_SIZE, INSUFFICIENT_ITER, BREAKDOWN = 0, 1, 2, 3, 4
LARGEST, SMALLEST = 0, 1
MAX_NCV = 64
MAX_SWEEPS = 30
EPS64 = float(np.finfo(np.float64).eps)

# Ts (keep_T): the projected matrices handed to the Jacobi routine, one per cycle; sweeps: the most sweeps any of them took
Result = namedtuple("Result", "status vals X res nconv restarts matvecs Ts sweeps")


def real_dtype(dt):
    return np.dtype(np.float32 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)


def default_tol(dt):
    return 1e-4 if real_dtype(dt) == np.dtype(np.float32) else 1e-10


def default_v0(n, dt):
    """What Eigsh.solve(v0=None) uses."""
    from sprsolve_amd import gen
    v = gen.uniform(gen.SEED, n, stream=90)
    if np.dtype(dt).kind == "c":
        v = v + 1j * gen.uniform(gen.SEED, n, stream=91)
    return v.astype(dt)


def restart_size(k, m):
    return min(k + max(k, 4), m - 2)


def dense(indptr, indices, data):
    import scipy.sparse as sp
    n = indptr.size - 1
    return sp.csr_matrix((data, indices, indptr), shape=(n, n)).toarray()


def _matvec(indptr, indices, data):
    import scipy.sparse as sp
    n = indptr.size - 1
    M = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    return lambda v: (M @ v).astype(data.dtype, copy=False)


def pairs(r, M):
    """Round r of the round-robin pairing of M (even) indices, each pair ordered p < q."""
    i = np.arange(1, M // 2)
    a = np.concatenate([[M - 1], (r + i) % (M - 1)]) if M > 2 else np.array([M - 1])
    b = np.concatenate([[r], (r - i) % (M - 1)]) if M > 2 else np.array([r])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi_eigh(T):
    """-> (theta, S, sweeps, converged): T = S diag(theta) S^T, unsorted, by the header's cyclic Jacobi in float64."""
    T = np.asarray(T, np.float64)
    me = T.shape[0]
    M = (me + 1) & ~1
    A = np.zeros((M, M)); A[:me, :me] = T
    S = np.eye(M)
    fro2 = float(np.sum(A * A))
    sweeps, conv = 0, False
    while True:
        B = A.copy(); np.fill_diagonal(B, 0.0)
        off2 = float(np.sum(B * B))
        if off2 <= EPS64 * EPS64 * fro2:
            conv = True
            break
        if sweeps == MAX_SWEEPS:
            break
        for r in range(M - 1):
            p, q = pairs(r, M)
            apq = A[p, q]
            nz = apq != 0.0
            with np.errstate(all="ignore"):
                tau = (A[q, q] - A[p, p]) / (2.0 * np.where(nz, apq, 1.0))
                t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = t * c
            c = np.where(nz, c, 1.0); s = np.where(nz, s, 0.0)
            for X in (A, S):
                xp, xq = X[:, p].copy(), X[:, q].copy()
                X[:, p] = c * xp - s * xq; X[:, q] = s * xp + c * xq
            xp, xq = A[p, :].copy(), A[q, :].copy()
            A[p, :] = c[:, None] * xp - s[:, None] * xq; A[q, :] = s[:, None] * xp + c[:, None] * xq
            A[p, q] = 0.0; A[q, p] = 0.0
        sweeps += 1
    return np.diag(A)[:me].copy(), S[:me, :me].copy(), sweeps, conv


def order(theta, which):
    """Descending (LARGEST) or ascending (SMALLEST), ties by index."""
    key = -theta if which == LARGEST else theta
    return np.argsort(key, kind="stable")


def eigsh(indptr, indices, data, k, which, v0, ncv, max_restarts, tol, keep_T=False):
    """-> Result.  data / v0 share the dtype under test; X has shape (k, n) (None on BREAKDOWN)."""
    T_ = np.dtype(data.dtype)
    R = real_dtype(T_)
    n = indptr.size - 1
    m = min(32, n) if ncv == 0 else int(ncv)
    assert 3 <= m <= min(MAX_NCV, n) and 1 <= k <= m - 2 and which in (LARGEST, SMALLEST) and max_restarts >= 1
    A = _matvec(indptr, indices, data)
    epsR = float(np.finfo(R).eps)
    zk = np.zeros(k)

    def norm(v):
        with np.errstate(all="ignore"):
            return R.type(np.sqrt(np.sum((v.real * v.real + v.imag * v.imag).astype(R), dtype=R)))

    v0 = np.asarray(v0, T_)
    beta0 = norm(v0)
    if not beta0 > 0:
        return Result(BREAKDOWN, zk, None, zk, 0, 0, 0, [], 0)
    V = np.zeros((m + 1, n), T_)
    V[0] = v0 * R.type(R.type(1) / beta0)
    Tm = np.zeros((m, m))
    j0, anorm, scale, matvecs = 0, 0.0, 0.0, 0
    Ts, most = [], 0
    p = restart_size(k, m)
    c = 0
    while True:
        c += 1
        m_eff, invariant, beta = m, False, 0.0
        for j in range(j0, m):
            with np.errstate(all="ignore"):
                w = A(V[j])
                matvecs += 1
                h = np.zeros(j + 1, T_)
                for _ in range(2):
                    cf = np.array([np.vdot(V[i], w) for i in range(j + 1)], T_)
                    for i in range(j + 1):
                        w = w + V[i] * T_.type(-cf[i])
                    h = h + cf
                bR = norm(w)
            beta = float(bR)
            if not beta >= 0.0:
                return Result(BREAKDOWN, zk, None, zk, 0, c, matvecs, Ts, most)
            tjj = float(h[j].real)
            Tm[j, j] = tjj
            scale = max(scale, abs(tjj))
            if beta <= 64.0 * epsR * scale:
                m_eff, invariant = j + 1, True
                break
            scale = max(scale, beta)
            if j + 1 < m:
                Tm[j + 1, j] = Tm[j, j + 1] = beta
            V[j + 1] = w * R.type(R.type(1) / bR)
        Tc = Tm[:m_eff, :m_eff].copy()
        if keep_T:
            Ts.append(Tc)
        theta, S, sweeps, conv = jacobi_eigh(Tc)
        most = max(most, sweeps)
        if not conv:
            return Result(BREAKDOWN, zk, None, zk, 0, c, matvecs, Ts, most)
        o = order(theta, which)
        theta, S = theta[o], S[:, o]
        res = beta * np.abs(S[m_eff - 1])
        anorm = max(anorm, float(np.max(np.abs(theta))))
        nconv = 0
        while nconv < min(k, m_eff) and res[nconv] <= tol * anorm:
            nconv += 1
        status = None
        if invariant:
            if m_eff < k:
                vals = np.zeros(k); vals[:m_eff] = theta
                rs = np.zeros(k); rs[:m_eff] = res
                return Result(BREAKDOWN, vals, None, rs, nconv, c, matvecs, Ts, most)
            status, nconv = OK, k
        elif nconv == k:
            status = OK
        elif c == max_restarts:
            status = INSUFFICIENT_ITER
        if status is not None:
            Sr = S[:, :k].astype(R).astype(T_)
            X = (V[:m_eff].T @ Sr).T.astype(T_)
            return Result(status, theta[:k].copy(), np.ascontiguousarray(X), res[:k].copy(), nconv, c, matvecs, Ts, most)
        Sr = S[:, :p].astype(R).astype(T_)
        V[:p] = (V[:m].T @ Sr).T
        V[p] = V[m]
        Tm[:] = 0.0
        Tm[np.arange(p), np.arange(p)] = theta[:p]
        Tm[p, :p] = Tm[:p, p] = beta * S[m - 1, :p]
        j0 = p
