"""The thick-restart Lanczos bidiagonalisation of include/sprsolve_hip.h (sprs_svds_*) restated in numpy, in the dtype under
test with the projected matrix B in float64: the checker of tests/test_svds_cpu.py and tests/test_gpu_svds.py.  The one-sided
Jacobi SVD follows the header rule for rule (round-robin pairs on the columns, rotate only where |c| > eps sqrt(a b), a sweep
without a rotation ends it).  Vector operations round once per operation in the dtype under test as the library's do; the sums
(dot products, norms, the rows of the matrix products and of P Y, Q X) associate differently, so nothing is compared bit for
bit against it."""
from collections import namedtuple

import numpy as np

from _eigsh_ref import pairs, real_dtype, restart_size  # noqa: F401  (the same pairing, types and kept count as Eigsh)

OK, INCOMPATIBLE_RHS_SIZE, INCOMPATIBLE_X_SIZE, INSUFFICIENT_ITER, BREAKDOWN = 0, 1, 2, 3, 4
LARGEST, SMALLEST = 0, 1
MAX_NCV = 64
MAX_SWEEPS = 30
EPS64 = float(np.finfo(np.float64).eps)

# Bs (keep_B): the projected matrices handed to the Jacobi routine, one per cycle; sweeps: the most sweeps any of them took
Result = namedtuple("Result", "status s U V res nconv restarts matvecs Bs sweeps")


def default_tol(dt):
    return 1e-4 if real_dtype(dt) == np.dtype(np.float32) else 1e-10


def default_v0(shape, dt):
    """What Svds.solve(v0=None) uses: min(rows, cols) entries."""
    from sprsolve_amd import gen
    n = min(shape)
    v = gen.uniform(gen.SEED, n, stream=92)
    if np.dtype(dt).kind == "c":
        v = v + 1j * gen.uniform(gen.SEED, n, stream=93)
    return v.astype(dt)


def matrix(shape, indptr, indices, data):
    import scipy.sparse as sp
    return sp.csr_matrix((data, indices, indptr), shape=shape)


def dense(shape, indptr, indices, data):
    """Duplicates of a column in a row are summed, as the SpMV sums them."""
    M = np.zeros(shape, dtype=np.complex128 if data.dtype.kind == "c" else np.float64)
    np.add.at(M, (np.repeat(np.arange(shape[0]), np.diff(indptr)), indices), data)
    return M


def jacobi_svd(B):
    """-> (sigma, X, Y, sweeps, converged): B = X diag(sigma) Y^T, unsorted, by the header's one-sided Jacobi in float64.
    sigma_i = |g_i| of G = B Y; a zero or NaN sigma reports converged = False, as does the sweep cap."""
    B = np.asarray(B, np.float64)
    me = B.shape[0]
    M = (me + 1) & ~1
    G = np.zeros((M, M)); G[:me, :me] = B
    Y = np.eye(M)
    sweeps, conv = 0, False
    while True:
        rotated = False
        for r in range(M - 1):
            p, q = pairs(r, M)
            with np.errstate(all="ignore"):
                a = np.sum(G[:, p] * G[:, p], axis=0); b = np.sum(G[:, q] * G[:, q], axis=0); c = np.sum(G[:, p] * G[:, q], axis=0)
                rot = np.abs(c) > EPS64 * np.sqrt(a * b)
                zeta = (b - a) / (2.0 * np.where(rot, c, 1.0))
                t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / np.sqrt(1.0 + t * t)
                sn = cs * t
            cs = np.where(rot, cs, 1.0); sn = np.where(rot, sn, 0.0)
            rotated = rotated or bool(np.any(rot))
            for Z in (G, Y):
                zp, zq = Z[:, p].copy(), Z[:, q].copy()
                Z[:, p] = cs * zp - sn * zq; Z[:, q] = sn * zp + cs * zq
        if not rotated:
            conv = True
            break
        sweeps += 1
        if sweeps == MAX_SWEEPS:
            break
    with np.errstate(all="ignore"):
        sigma = np.sqrt(np.sum(G[:me, :me] * G[:me, :me], axis=0))
        if not np.all(sigma > 0.0):
            conv = False
        X = G[:me, :me] / sigma
    return sigma, X, Y[:me, :me].copy(), sweeps, conv


def order(sigma, which):
    """Descending (LARGEST) or ascending (SMALLEST), ties by index."""
    key = -sigma if which == LARGEST else sigma
    return np.argsort(key, kind="stable")


def svds(shape, indptr, indices, data, k, which, v0, ncv, max_restarts, tol, keep_B=False):
    """-> Result.  data / v0 share the dtype under test; U has shape (k, rows) and V (k, cols) (None on BREAKDOWN)."""
    T_ = np.dtype(data.dtype)
    R = real_dtype(T_)
    rows, cols = shape
    N, Mlen = min(rows, cols), max(rows, cols)
    m = min(32, N) if ncv == 0 else int(ncv)
    assert 3 <= m <= min(MAX_NCV, N) and 1 <= k <= m - 2 and which in (LARGEST, SMALLEST) and max_restarts >= 1
    A = matrix(shape, indptr, indices, data)
    AH = A.conj().T.tocsr()
    swap = rows < cols                                   # Op is M x N with M >= N: A, or A^H where A is wide
    Op_, OpH_ = (AH, A) if swap else (A, AH)
    Op = lambda v: (Op_ @ v).astype(T_, copy=False)
    OpH = lambda v: (OpH_ @ v).astype(T_, copy=False)
    epsR = float(np.finfo(R).eps)
    zk = np.zeros(k)

    def norm(v):
        with np.errstate(all="ignore"):
            return R.type(np.sqrt(np.sum((v.real * v.real + v.imag * v.imag).astype(R), dtype=R)))

    def cgs2(w, basis, cnt):
        for _ in range(2):
            cf = np.array([np.vdot(basis[i], w) for i in range(cnt)], T_)
            for i in range(cnt):
                w = w + basis[i] * T_.type(-cf[i])
        return w

    def done(status, sig, res, nconv, c, X=None, Y=None, me=0):
        s = np.zeros(k); rs = np.zeros(k)
        s[: min(k, sig.size)] = sig[:k]; rs[: min(k, res.size)] = res[:k]
        U = V = None
        if X is not None:
            Vv = (Pb[:me].T @ Y[:, :k].astype(R).astype(T_)).T.astype(T_)
            Uu = (Qb[:me].T @ X[:, :k].astype(R).astype(T_)).T.astype(T_)
            U, V = (Vv, Uu) if swap else (Uu, Vv)
            U, V = np.ascontiguousarray(U), np.ascontiguousarray(V)
        return Result(status, s, U, V, rs, nconv, c, matvecs, Bs, most)

    v0 = np.asarray(v0, T_)
    assert v0.size == N
    matvecs, Bs, most = 0, [], 0
    none = np.zeros(0)
    beta0 = norm(v0)
    if not beta0 > 0:
        return done(BREAKDOWN, none, none, 0, 0)
    Pb = np.zeros((m + 1, N), T_); Qb = np.zeros((m, Mlen), T_)
    Pb[0] = v0 * R.type(R.type(1) / beta0)
    Bm = np.zeros((m, m))
    j0, anorm, scale = 0, 0.0, 0.0
    sig = res = none
    nconv = 0
    p = restart_size(k, m)
    c = 0
    while True:
        c += 1
        m_eff, invariant, beta = m, False, 0.0
        for j in range(j0, m):
            with np.errstate(all="ignore"):
                w = cgs2(Op(Pb[j]), Qb, j)
                matvecs += 1
                aR = norm(w)
            alpha = float(aR)
            if not alpha >= 0.0 or alpha <= 64.0 * epsR * scale:      # NaN, or Op is rank-deficient along the basis
                return done(BREAKDOWN, sig, res, nconv, c)
            Bm[j, j] = alpha
            scale = max(scale, alpha)
            with np.errstate(all="ignore"):
                Qb[j] = w * R.type(R.type(1) / aR)
                w = cgs2(OpH(Qb[j]), Pb, j + 1)
                matvecs += 1
                bR = norm(w)
            beta = float(bR)
            if not beta >= 0.0:
                return done(BREAKDOWN, sig, res, nconv, c)
            if beta <= 64.0 * epsR * scale:
                m_eff, invariant, beta = j + 1, True, 0.0
                break
            scale = max(scale, beta)
            if j + 1 < m:
                Bm[j, j + 1] = beta
            Pb[j + 1] = w * R.type(R.type(1) / bR)
        Bc = Bm[:m_eff, :m_eff].copy()
        if keep_B:
            Bs.append(Bc)
        sigma, X, Y, sweeps, conv = jacobi_svd(Bc)
        most = max(most, sweeps)
        if not conv:
            return done(BREAKDOWN, sig, res, nconv, c)
        o = order(sigma, which)
        sig, X, Y = sigma[o], X[:, o], Y[:, o]
        res = beta * np.abs(X[m_eff - 1])
        anorm = max(anorm, float(np.max(sig)))
        nconv = 0
        while nconv < min(k, m_eff) and res[nconv] <= tol * anorm:
            nconv += 1
        if invariant:
            if m_eff < k:
                return done(BREAKDOWN, sig, res, nconv, c)
            return done(OK, sig, res, k, c, X, Y, m_eff)
        if nconv == k:
            return done(OK, sig, res, nconv, c, X, Y, m_eff)
        if c == max_restarts:
            return done(INSUFFICIENT_ITER, sig, res, nconv, c, X, Y, m_eff)
        Pb[:p] = (Pb[:m].T @ Y[:, :p].astype(R).astype(T_)).T
        Qb[:p] = (Qb[:m].T @ X[:, :p].astype(R).astype(T_)).T
        Pb[p] = Pb[m]
        Bm[:] = 0.0
        Bm[np.arange(p), np.arange(p)] = sig[:p]
        Bm[:p, p] = beta * X[m - 1, :p]
        j0 = p
