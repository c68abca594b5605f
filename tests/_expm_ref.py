"""The Krylov propagator w = exp(tA) v of include/sprsolve_hip.h (sprs_expm_*) restated in numpy, in the dtype under test with
the projected matrix H, the small exponential F, every tau and the error estimates in float64 / complex128: the checker of
tests/test_expm_cpu.py and tests/test_gpu_expm.py.  round2 and smallexp follow the header operation by operation (the matrix
products sum over the inner index ascending, one product and one sum per term).  Vector operations round once per operation in
the dtype under test as the library's do; the sums over a vector's length (dot products, norms, the rows of the matrix product)
associate differently, so nothing is compared bit for bit against it.  sums="pairwise" forms the dot products and norms with
numpy's pairwise sums instead of BLAS's order: the two differ by what a summation order may change."""
from collections import namedtuple

import numpy as np

OK, INCOMPATIBLE_RHS_SIZE, INCOMPATIBLE_X_SIZE, INSUFFICIENT_ITER, BREAKDOWN = 0, 1, 2, 3, 4
MAX_NCV = 48
DEFAULT_NCV = 30
HORNER = 18
MAX_SQUARINGS = 64
MAX_REJECTS = 10
GAMMA, DELTA = 0.9, 1.2
DBL_MIN = float(np.finfo(np.float64).tiny)

# Hs (keep_H): per sub-step (the matrix handed to smallexp at the accepted tau_s, without the factor sgn tau_s; tau_s; sgn)
Result = namedtuple("Result", "status w err hump t_done steps rejects matvecs m_effs Hs")


def real_dtype(dt):
    return np.dtype(np.float32 if np.dtype(dt) in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)


def wide_dtype(dt):
    return np.dtype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)


def default_tol(dt):
    return float(np.sqrt(np.finfo(real_dtype(dt)).eps))


def start_vector(n, dt):
    """The start vector of the tests: gen.uniform(7, n), stream 1 for the imaginary part."""
    from sprsolve_amd import gen
    v = gen.uniform(7, n)
    if np.dtype(dt).kind == "c":
        v = v + 1j * gen.uniform(7, n, stream=1)
    return v.astype(dt)


def dense(indptr, indices, data):
    import scipy.sparse as sp
    n = indptr.size - 1
    return sp.csr_matrix((data, indices, indptr), shape=(n, n)).toarray()


def _matvec(indptr, indices, data):
    import scipy.sparse as sp
    n = indptr.size - 1
    M = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    return lambda v: (M @ v).astype(data.dtype, copy=False)


def round2(x):
    """x to two significant decimal digits, as Expokit rounds its step sizes: floor(y + 0.55) 10^u with y = x 10^-u in
    [10, 100), u reached by dividing or multiplying by ten one step at a time (330 at the most) and undone the same way.
    Anything that is not a finite positive number is returned as it is."""
    x = float(x)
    if not (x > 0.0) or x == np.inf:
        return x
    y, u = x, 0
    for _ in range(330):
        if not y >= 100.0:
            break
        y = y / 10.0; u += 1
    for _ in range(330):
        if not y < 10.0:
            break
        y = y * 10.0; u -= 1
    r = float(np.floor(y + 0.55))
    for _ in range(abs(u)):
        r = r * 10.0 if u > 0 else r / 10.0
    return r


def _mulr(Z, f):
    """Z f for a real f: every real and imaginary part times f, rounded once."""
    Z = np.ascontiguousarray(Z)
    if Z.dtype.kind == "c":
        return (Z.view(np.float64) * float(f)).view(np.complex128)
    return Z * float(f)


def _divr(Z, q):
    Z = np.ascontiguousarray(Z)
    if Z.dtype.kind == "c":
        return (Z.view(np.float64) / float(q)).view(np.complex128)
    return Z / float(q)


def _mm(A, B):
    """A B with every entry summed over the inner index ascending, one product and one sum per term."""
    acc = np.zeros((A.shape[0], B.shape[1]), A.dtype)
    for j in range(A.shape[1]):
        acc = acc + A[:, j:j + 1] * B[j:j + 1, :]
    return acc


def smallexp(X):
    """-> (F, s), or (None, s) where the header says SPRS_BREAKDOWN: Taylor scaling and squaring of degree 18."""
    X = np.asarray(X)
    X = X.astype(np.complex128 if X.dtype.kind == "c" else np.float64)
    M = X.shape[0]
    with np.errstate(all="ignore"):
        col = np.zeros(M)
        for i in range(M):
            col = col + np.abs(X[i, :])
        nrm = float(np.max(col)) if M else 0.0
        if not np.isfinite(nrm):
            return None, 0
        s, x, g = 0, nrm, 1.0
        while s < MAX_SQUARINGS and x > 0.5:
            x *= 0.5; g *= 0.5; s += 1
        if x > 0.5:
            return None, s
        Y = _mulr(X, g)
        I = np.eye(M, dtype=X.dtype)
        E = I.copy()
        for q in range(HORNER, 0, -1):
            E = I + _divr(_mm(Y, E), q)
        for _ in range(s):
            E = _mm(E, E)
    return E, s


def expm_apply(indptr, indices, data, t, v, ncv=0, tol=0.0, max_steps=100000, tau0=0.0, keep_H=False, sums="blas"):
    """-> Result.  data / v share the dtype under test; w is None on BREAKDOWN."""
    T_ = np.dtype(data.dtype)
    R = real_dtype(T_)
    W = wide_dtype(T_)
    n = indptr.size - 1
    m = min(DEFAULT_NCV, n) if ncv == 0 else int(ncv)
    assert 3 <= m <= min(MAX_NCV, n) and np.isfinite(t) and max_steps >= 1 and tol >= 0.0 and tau0 >= 0.0 and np.isfinite(tau0)
    A = _matvec(indptr, indices, data)
    epsR = float(np.finfo(R).eps)
    tol = float(tol) if tol != 0.0 else default_tol(T_)
    v = np.asarray(v, T_)

    def norm(x):
        with np.errstate(all="ignore"):
            return R.type(np.sqrt(np.sum((x.real * x.real + x.imag * x.imag).astype(R), dtype=R)))

    def cdot(a, b):
        if sums == "pairwise":
            return T_.type(np.sum(np.conj(a) * b, dtype=T_))
        return T_.type(np.vdot(a, b))

    t = float(R.type(t))
    sgn, t_out = (1.0 if t >= 0 else -1.0), abs(t)
    if t_out == 0.0:
        return Result(OK, v.copy(), 0.0, 0.0, 0.0, 0, 0, 0, [], [])
    t_now, tau, hump, err_sum = 0.0, float(tau0), 0.0, 0.0
    steps = rejects = matvecs = 0
    w = v.copy()
    m_effs, Hs = [], []

    def out(status, w_):
        return Result(status, w_, err_sum, hump, sgn * t_now, steps, rejects, matvecs, m_effs, Hs)

    with np.errstate(all="ignore"):
        while True:
            bR = norm(w)
            beta = float(bR)
            if not beta >= 0.0:
                return out(BREAKDOWN, None)
            if beta == 0.0:
                return out(OK, np.zeros(n, T_))
            hump = max(hump, beta)
            V = np.zeros((m + 1, n), T_)
            V[0] = w * R.type(R.type(1) / bR)
            H = np.zeros((m + 2, m + 2), W)
            scale, m_eff, happy = 0.0, m, False
            for j in range(m):
                p = A(V[j])
                matvecs += 1
                h = np.zeros(j + 1, T_)
                for _ in range(2):
                    cf = np.array([cdot(V[i], p) for i in range(j + 1)], T_)
                    for i in range(j + 1):
                        p = p + V[i] * T_.type(-cf[i])
                    h = h + cf
                H[:j + 1, j] = h.astype(W)
                hR = norm(p)
                hn = float(hR)
                if not hn >= 0.0:
                    return out(BREAKDOWN, None)
                scale = max(scale, float(np.max(np.abs(H[:j + 1, j]))))
                if hn <= 64.0 * epsR * scale:
                    m_eff, happy = j + 1, True
                    break
                scale = max(scale, hn)
                H[j + 1, j] = hn
                V[j + 1] = p * R.type(R.type(1) / hR)
            rem = t_out - t_now
            if happy:
                tau_s, err, xm = rem, 0.0, 0.0
                Hc = H[:m_eff, :m_eff]
                F, _ = smallexp(_mulr(Hc, sgn * tau_s))
                if F is None:
                    return out(BREAKDOWN, None)
                ncoef = m_eff
            else:
                avnorm = float(norm(A(V[m])))
                matvecs += 1
                H[m + 1, m] = 1.0
                if tau == 0.0:
                    row = np.zeros(m + 1)
                    for c in range(m):
                        row = row + np.abs(H[:m + 1, c])
                    anorm = float(np.max(row))
                    fact = ((m + 1) / np.e) ** (m + 1) * np.sqrt(2.0 * np.pi * (m + 1))
                    tau = round2((1.0 / anorm) * ((fact * tol) / (4.0 * beta * anorm)) ** (1.0 / m))
                tau_s = tau if tau < rem else rem
                Hc = H
                k = 0
                while True:
                    F, _ = smallexp(_mulr(Hc, sgn * tau_s))
                    if F is None:
                        return out(BREAKDOWN, None)
                    e1 = beta * float(np.abs(F[m, 0]))
                    e2 = beta * float(np.abs(F[m + 1, 0])) * avnorm
                    if e1 > 10.0 * e2:
                        err, xm = e2, 1.0 / m
                    elif e1 > e2:
                        err, xm = e1 * e2 / (e1 - e2), 1.0 / m
                    else:
                        err, xm = e1, 1.0 / (m - 1)
                    if err != err:
                        return out(BREAKDOWN, None)
                    if err <= DELTA * tau_s * tol:
                        break
                    if k == MAX_REJECTS - 1:
                        return out(BREAKDOWN, None)
                    tau_s = round2(GAMMA * tau_s * (tau_s * tol / err) ** xm)
                    rejects += 1; k += 1
                    if not (tau_s > 0.0) or tau_s == np.inf:
                        return out(BREAKDOWN, None)
                tau = round2(GAMMA * tau_s * (tau_s * tol / max(err, DBL_MIN)) ** xm)
                ncoef = m + 1
            if keep_H:
                Hs.append((Hc.copy(), tau_s, sgn))
            c = _mulr(F[:ncoef, 0], beta).astype(T_)
            w = np.zeros(n, T_)
            for i in range(ncoef):
                w = w + V[i] * c[i]
            t_now = t_out if tau_s == rem else t_now + tau_s
            err_sum += err
            steps += 1
            m_effs.append(m_eff)
            if t_now >= t_out:
                return out(OK, w)
            if steps == max_steps:
                return out(INSUFFICIENT_ITER, w)
