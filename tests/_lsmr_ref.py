"""The LSMR recurrence of include/sprsolve_hip.h (sprs_lsmr_*) restated in numpy, step for step (V1 - V4, S1 - S8, T), in the
dtype under test: the checker of tests/test_lsmr_cpu.py and tests/test_gpu_lsmr.py, and the generator of their test systems.
Every recurrence scalar is real and of the dtype's real type; u is kept un-normalised as the header says.  Only the sums (norms,
the row sums of the matrix products) associate differently from the library's, so nothing is compared bit for bit against it."""
from collections import namedtuple

import numpy as np

OK, INSUFFICIENT_ITER, BREAKDOWN, DIM_MISMATCH, INVALID_ARGUMENT = 0, 3, 4, 6, 7

Result = namedtuple("Result", "status its res ares x trace")     # trace: rows (its, normr, normar, alpha, beta, normA)


def system(m, n, dtype, seed=0, consistent=True):
    """-> (indptr, indices, data, rhs): row i has 1 + (i mod 5) entries, one of them at column i mod n with 4 added to its
    U(-1, 1) value, the others at random columns (duplicates of a column may occur and are kept); complex dtypes get a random
    imaginary part.  consistent: rhs = A xs for a random xs, else a random vector."""
    rng = np.random.default_rng(seed)
    T = np.dtype(dtype)
    cnt = 1 + np.arange(m) % 5
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    nnz = int(indptr[-1])
    indices = rng.integers(0, n, nnz).astype(np.int32)
    data = rng.uniform(-1, 1, nnz)
    if T.kind == "c":
        data = data + 1j * rng.uniform(-1, 1, nnz)
    first = indptr[:-1]
    indices[first] = np.arange(m) % n
    data[first] += 4.0
    for i in range(m):                                             # a row's columns in ascending order, as CSR usually has them
        a, b = indptr[i], indptr[i + 1]
        o = np.argsort(indices[a:b], kind="stable")
        indices[a:b] = indices[a:b][o]; data[a:b] = data[a:b][o]
    data = data.astype(T)
    if consistent:
        xs = rng.uniform(-1, 1, n) + (1j * rng.uniform(-1, 1, n) if T.kind == "c" else 0)
        rhs = (matrix(m, n, indptr, indices, data) @ xs).astype(T)
    else:
        rhs = (rng.uniform(-1, 1, m) + (1j * rng.uniform(-1, 1, m) if T.kind == "c" else 0)).astype(T)
    return indptr, indices, data, rhs


def matrix(m, n, indptr, indices, data):
    import scipy.sparse as sp
    return sp.csr_matrix((data, indices, indptr), shape=(m, n))


def dense(m, n, indptr, indices, data):
    M = np.zeros((m, n), dtype=np.complex128 if data.dtype.kind == "c" else np.float64)
    np.add.at(M, (np.repeat(np.arange(m), np.diff(indptr)), indices), data)
    return M


def _sign(R, a):
    return R.type(1) if a > 0 else (R.type(-1) if a < 0 else R.type(0))


def symortho(R, a, b):
    one = R.type(1)
    if b == 0:
        return _sign(R, a), R.type(0), abs(a)
    if a == 0:
        return R.type(0), _sign(R, b), abs(b)
    if abs(b) > abs(a):
        tau = a / b
        s = _sign(R, b) / np.sqrt(one + tau * tau)
        c = s * tau
        return c, s, b / s
    tau = b / a
    c = _sign(R, a) / np.sqrt(one + tau * tau)
    s = c * tau
    return c, s, a / c


def lsmr(shape, indptr, indices, data, rhs, x0, max_iter, tol, damp=0.0):
    """-> Result.  data / rhs / x0 share the dtype under test.  res, ares are what the library reports in *res_out, *ares_out."""
    T = np.dtype(data.dtype)
    R = np.dtype(np.float32 if T in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)
    m, n = shape
    rhs = np.asarray(rhs, dtype=T); x = np.array(x0, dtype=T)
    if rhs.size != m or x.size != n:
        return Result(DIM_MISMATCH, 0, 0.0, 0.0, x, [])
    if not damp >= 0:
        return Result(INVALID_ARGUMENT, 0, 0.0, 0.0, x, [])
    M = matrix(m, n, indptr, indices, data)
    MH = M.conj().T.tocsr()
    A = lambda p: (M @ p).astype(T, copy=False)
    AH = lambda p: (MH @ p).astype(T, copy=False)
    norm2 = lambda p: R.type(np.linalg.norm(p))
    one, zero = R.type(1), R.type(0)
    tol = R.type(tol); damp = R.type(damp)
    finite = np.isfinite
    trace = []
    with np.errstate(all="ignore"):
        normb = norm2(rhs)
        if normb <= np.finfo(R).eps:
            return Result(OK, 0, float(normb), 0.0, np.zeros(n, T), trace)
        u = rhs * one + A(x) * (-one)
        beta = norm2(u)
        if not finite(beta):
            return Result(BREAKDOWN, 0, 0.0, 0.0, x, trace)
        if beta == 0:
            return Result(OK, 0, 0.0, 0.0, x, trace)
        v = AH(u)
        v = v * (one / beta)
        alpha = norm2(v)
        if not finite(alpha):
            return Result(BREAKDOWN, 0, 0.0, 0.0, x, trace)
        if alpha == 0:
            return Result(OK, 0, float(beta / normb), 0.0, x, trace)
        v = v * (one / alpha)
        h = v.copy(); hbar = np.zeros(n, T)
        alphabar = alpha; zetabar = alpha * beta; rho = rhobar = cbar = one; sbar = zero
        betadd = beta; betad = zero; rhodold = one; tautildeold = thetatilde = zeta = d = zero
        normA2 = alpha * alpha
        for its in range(max_iter):
            f = -(alpha * (one / beta))                                     # V1
            u = A(v) * one + u * f
            beta = norm2(u)                                                 # V2
            if not finite(beta):
                return Result(BREAKDOWN, its, 0.0, 0.0, x, trace)
            if beta > 0:                                                    # V3
                v = AH(u) * (one / beta) + v * (-beta)
                alpha = norm2(v)
                if not finite(alpha):
                    return Result(BREAKDOWN, its, 0.0, 0.0, x, trace)
            else:
                alpha = zero
            chat, shat, alphahat = symortho(R, alphabar, damp)              # S1
            rhoold = rho
            c, s, rho = symortho(R, alphahat, beta)
            thetanew = s * alpha; alphabar = c * alpha                      # S2
            rhobarold = rhobar; zetaold = zeta; thetabar = sbar * rho
            cbar, sbar, rhobar = symortho(R, cbar * rho, thetanew)          # S3
            zeta = cbar * zetabar; zetabar = -sbar * zetabar
            g1 = -(thetabar * rho / (rhoold * rhobarold))                   # S4
            g2 = zeta / (rho * rhobar)
            g3 = -(thetanew / rho)
            betaacute = chat * betadd; betacheck = -shat * betadd           # S5
            betahat = c * betaacute; betadd = -s * betaacute
            thetatildeold = thetatilde                                      # S6
            ct, st, rt = symortho(R, rhodold, thetabar)
            thetatilde = st * rhobar; rhodold = ct * rhobar
            betad = -st * betad + ct * betahat
            tautildeold = (zetaold - thetatildeold * tautildeold) / rt
            taud = (zeta - thetatilde * tautildeold) / rhodold
            d = d + betacheck * betacheck
            dt = betad - taud                                               # S7
            normr = np.sqrt(d + dt * dt + betadd * betadd)
            normA2 = normA2 + beta * beta
            normA = np.sqrt(normA2)
            normA2 = normA2 + alpha * alpha
            normar = abs(zetabar)
            if not all(finite(q) for q in (g1, g2, g3, normr, normA, normar)):   # S8
                return Result(BREAKDOWN, its, 0.0, 0.0, x, trace)
            hbar = h * one + hbar * g1                                      # V4
            x = x + hbar * g2
            if alpha > 0:
                v = v * (one / alpha)
            h = v * one + h * g3
            normx = norm2(x)                                                # T
            trace.append((its, float(normr), float(normar), float(alpha), float(beta), float(normA)))
            if beta == 0 or alpha == 0 or normr <= tol * normb + tol * normA * normx or normar <= tol * normA * normr:
                dn = normA * normr
                return Result(OK, its + 1, float(normr / normb), float(normar / dn) if dn > 0 else 0.0, x, trace)
    return Result(INSUFFICIENT_ITER, max_iter, 0.0, 0.0, x, trace)


def trace_array(trace):
    """The rows in the library's 8-double layout: [its, normr, normar, 0, alpha, 0, beta, 0]."""
    return np.array([[t[0], t[1], t[2], 0.0, t[3], 0.0, t[4], 0.0] for t in trace]).reshape(-1, 8)
