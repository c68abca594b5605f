"""The IDR(s) recurrence of include/sprsolve_hip.h (sprs_idrs_*) restated in numpy, op for op, in the dtype under test, with the
small quantities (M, f, c, alpha, beta, q, omega) and every dot product as Python floats / complex numbers (doubles, as in the library): the checker of
tests/test_idrs_cpu.py and tests/test_gpu_idrs.py.  Every vector op rounds once per element operation as the library's kernels
do; only the sums (the dot products, the norms, the row sums of the matrix product) associate differently, so nothing is
compared bit for bit against it.  `order`: a permutation of range(n) in which every dot product and norm takes its sum — what a
change of summation order does to the iterates."""
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_ref as ref  # noqa: E402

OK, INSUFFICIENT_ITER, BREAKDOWN = ref.OK, ref.INSUFFICIENT_ITER, ref.BREAKDOWN
MAX_S = 8

# trace: the library's rows [its, rn before the step, re, im of beta / omega, re, im of M_kk / tt, k (s: the omega step), 0];
# rns[i]: |r| after i products with A (the recursive residual the events are taken on)
Result = namedtuple("Result", "status its res x trace rns")


def real_of(T):
    T = np.dtype(T)
    return np.dtype(np.float32 if T in (np.dtype(np.float32), np.dtype(np.complex64)) else np.float64)


def wide_of(T):
    return np.dtype(np.complex128 if np.dtype(T).kind == "c" else np.float64)


def shadow(n, s, dtype):
    """The library's shadow space: column c = gen.uniform(SEED, n, stream=200 + 2c) (+ 1j * stream 201 + 2c) rounded to the dtype,
    then, in double, orthonormalised by CGS2 against the earlier columns and scaled by 1 / norm2; rounded to the dtype at the end.
    -> (s, n) array, row c = p_c."""
    from sprsolve_amd import gen
    T = np.dtype(dtype); R = real_of(T); W = wide_of(T)
    P = np.zeros((s, n), W)
    for c in range(s):
        w = gen.uniform(gen.SEED, n, stream=200 + 2 * c).astype(R)
        if T.kind == "c":
            w = (w + 1j * gen.uniform(gen.SEED, n, stream=201 + 2 * c).astype(R)).astype(T)
        w = w.astype(T).astype(W)
        for _ in range(2 if c else 0):
            h = [np.vdot(P[i], w) for i in range(c)]
            for i in range(c):
                w = w + P[i] * (-h[i])
        P[c] = w * (1.0 / float(np.sqrt(np.vdot(w, w).real)))
    return P.astype(T)


def idrs(A, rhs, x0, max_iter, tol, s=4, precond_diag=None, kappa=0.7, P=None, order=None):
    """-> Result.  A: (indptr, indices, data) or a dense matrix, of the dtype under test, as rhs and x0; precond_diag (the matrix
    diagonal handed to DiagPrecond, real or of the dtype) or None; P: an explicit (s, n) shadow space (rows p_c) instead of the
    library's.  `res` is what the library reports in *res_out."""
    if not isinstance(A, tuple):                           # dense: as CSR with every entry stored
        A = np.asarray(A)
        nn = A.shape[0]
        A = (np.arange(0, nn * nn + 1, nn, dtype=np.int32), np.tile(np.arange(nn, dtype=np.int32), nn), np.ascontiguousarray(A.ravel()))
    T = np.dtype(A[2].dtype)
    n = A[0].size - 1
    R = real_of(T); W = wide_of(T)
    cx = T.kind == "c"

    def mul(a, b):
        """a * b per element in the library's formulas (csrc/scalar.hpp): for complex operands the naive product, every real
        operation rounded once — numpy's own complex loops may fuse a multiply and an add."""
        if not cx:
            return a * b
        a = np.asarray(a, T); b = np.asarray(b, T)
        ar, ai, br, bi = a.real, a.imag, b.real, b.imag
        out = np.empty(np.broadcast(a, b).shape, T)
        out.real = ar * br - ai * bi
        out.imag = ar * bi + ai * br
        return out

    if cx:
        import scipy.sparse as sp
        ip_, ix_, d_ = A
        ones = np.ones(n, R)

        def mv(v):                                         # x[col] * val in the naive formula, summed along the row in order
            prod = mul(v[ix_], d_)
            out = np.empty(n, T)
            out.real = sp.csr_matrix((np.ascontiguousarray(prod.real), ix_, ip_), shape=(n, n)) @ ones
            out.imag = sp.csr_matrix((np.ascontiguousarray(prod.imag), ix_, ip_), shape=(n, n)) @ ones
            return out
    else:
        mv = ref._matvec(*A)
    D = complex if cx else float
    rhs = np.asarray(rhs, dtype=T); x = np.array(x0, dtype=T)
    one = T.type(1)
    if s == 0:
        s = 4
    assert 1 <= s <= MAX_S and s <= n
    dinv = None
    if precond_diag is not None:
        d = np.asarray(precond_diag)
        if d.dtype.kind == "c":                            # DiagPrecond::new: V::one() / v in V, the library's naive quotient
            nn = d.real * d.real + d.imag * d.imag
            dinv = np.empty(d.shape, d.dtype)
            dinv.real = d.real / nn
            dinv.imag = -d.imag / nn
        else:
            dinv = d.dtype.type(1) / d
    prec = (lambda v: mul(v, dinv.astype(T) if cx else dinv).astype(T)) if dinv is not None else (lambda v: v)
    if order is None:
        pick = lambda v: v
    else:
        pick = lambda v: v[order]
    norm2 = lambda v: R.type(np.linalg.norm(pick(v)))
    # sum conj(a_i) b_i in double: the operands are widened, so for f32 / c32 every product is exact and only the sum rounds
    cdot = lambda a, b: np.vdot(pick(a).astype(W), pick(b).astype(W))
    sumsq = lambda v: float(np.vdot(pick(v).astype(W), pick(v).astype(W)).real)
    P = shadow(n, s, T) if P is None else np.asarray(P, dtype=T).reshape(s, n)
    trace = []; rns = []

    rhs_norm = norm2(rhs)
    if rhs_norm <= np.finfo(R).eps:
        return Result(OK, 0, float(rhs_norm), np.zeros(n, T), trace, rns)
    tol2 = R.type(tol) * rhs_norm
    r = mv(x)
    r = rhs * one + r * (-one)
    r0 = norm2(r)
    if r0 <= tol2:
        return Result(OK, 0, float(r0 / rhs_norm), x, trace, [float(r0)])
    G = np.zeros((s, n), T); U = np.zeros((s, n), T)
    M = [[D(1.0) if i == j else D(0.0) for j in range(s)] for i in range(s)]
    omega = D(1.0)
    sN = float(r0) * float(r0)
    its = 0
    rn = r0

    def decide():
        """The events a step begins with; None: the solve goes on."""
        nonlocal rn
        rn = float(np.sqrt(sN))
        rns.append(float(rn))
        if not np.isfinite(rn):
            return Result(BREAKDOWN, its, 0.0, x, trace, rns)
        if rn <= float(tol2):
            return Result(OK, its, float(R.type(rn / float(rhs_norm))), x, trace, rns)
        if its >= max_iter:
            return Result(INSUFFICIENT_ITER, max_iter, 0.0, x, trace, rns)
        return None

    with np.errstate(all="ignore"):
        while True:
            f = [D(cdot(P[i], r)) for i in range(s)]
            for k in range(s):
                ev = decide()
                if ev is not None:
                    return ev
                c = [D(0.0)] * s
                for i in range(k, s):                      # M[k:,k:] c = f[k:], forward
                    t = f[i]
                    for j in range(k, i):
                        t = t - M[i][j] * c[j]
                    c[i] = t / M[i][i] if M[i][i] != 0 else D(np.nan)
                v = r
                w = np.zeros(n, T)
                for i in range(k, s):
                    cT = T.type(c[i])
                    v = v + mul(G[i], -cT)
                    w = w + mul(U[i], cT)
                vh = prec(v)
                U[k] = mul(vh, T.type(omega)) + w
                G[k] = mv(U[k])
                its += 1
                q = [D(cdot(P[i], G[k])) for i in range(s)]
                alpha = [D(0.0)] * k
                for i in range(k):                         # M[:k,:k] alpha = q[:k], forward
                    t = q[i]
                    for j in range(i):
                        t = t - M[i][j] * alpha[j]
                    alpha[i] = t / M[i][i] if M[i][i] != 0 else D(np.nan)
                col = [D(0.0)] * s
                for i in range(k, s):
                    m = q[i]
                    for j in range(k):
                        m = m - M[i][j] * alpha[j]
                    col[i] = m
                if not np.isfinite(col[k]) or col[k] == 0:
                    return Result(BREAKDOWN, its, 0.0, x, trace, rns)
                gk = G[k]; uk = U[k]
                for i in range(k):
                    na = -T.type(alpha[i])
                    gk = gk + mul(G[i], na)
                    uk = uk + mul(U[i], na)
                G[k] = gk; U[k] = uk
                for i in range(k, s):
                    M[i][k] = col[i]
                beta = f[k] / col[k]
                bT = T.type(beta)
                r = r + mul(gk, -bT)
                x = x + mul(uk, bT)
                for i in range(k + 1, s):
                    f[i] = f[i] - beta * col[i]
                sN = sumsq(r)
                trace.append((its, float(rn), complex(beta), complex(col[k]), k))
            ev = decide()
            if ev is not None:
                return ev
            vh = prec(r)
            t = mv(vh)
            its += 1
            tt = float(cdot(t, t).real)
            tr = D(cdot(t, r))
            rho = abs(tr) / (np.sqrt(tt) * float(rn)) if tt > 0 else np.nan
            omega = tr * (1.0 / tt) if tt != 0 else D(np.nan)
            if rho < kappa:
                omega = omega * (kappa / rho)
            if not (tt > 0 and np.isfinite(tt) and np.isfinite(omega) and omega != 0):
                return Result(BREAKDOWN, its, 0.0, x, trace, rns)
            oT = T.type(omega)
            x = x + mul(vh, oT)
            r = r + mul(t, -oT)
            sN = sumsq(r)
            trace.append((its, float(rn), complex(omega), complex(tt), s))


def trace_array(trace):
    """The rows in the library's 8-double layout."""
    return np.array([[t[0], t[1], t[2].real, t[2].imag, t[3].real, t[3].imag, t[4], 0.0] for t in trace], dtype=np.float64).reshape(-1, 8)



# ---- the inputs the GPU tests solve, shared with the CPU self-check of their margins
F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64


def tol_of(dt):
    return 1e-5 if np.dtype(dt) in (np.dtype(F32), np.dtype(C32)) else 1e-10


def system(name, dt):
    """-> (indptr, indices, data, rhs, jacobi diagonal) in dtype dt; rhs = gen.uniform(7, n) for the convection-diffusion grids."""
    from sprsolve_amd import gen
    dt = np.dtype(dt)
    if name == "csg9x8":
        ip, ix, d, rhs, diag = gen.complex_symmetric_grid(9, 8)
        return ip, ix, d.astype(dt), rhs.astype(dt), diag.astype(dt)
    args = {"cd12x11": (12, 11, 0.3, 0.2), "cd24x22": (24, 22, 2.0, 1.5), "cd31x29": (31, 29, 0.3, 0.2), "cd96x90": (96, 90, 0.3, 0.2),
            "cd24x22m": (24, 22, 0.3, 0.2)}[name]
    ip, ix, d = gen.convection_diffusion_2d(args[0], args[1], cx=args[2], cy=args[3])[:3]
    n = ip.size - 1
    rhs = gen.uniform(7, n)
    diag = np.full(n, 4.0)
    R = real_of(dt)
    return ip, ix, d.astype(dt), rhs.astype(dt), diag.astype(R)


# (system, dtype, s, jacobi) of tests 1 - 3 of tests/test_gpu_idrs.py
FOLLOW = ([("cd12x11", dt, s, pc) for dt in (F64, F32) for s in (1, 4, 8) for pc in (False, True)]
          + [("csg9x8", dt, s, pc) for dt in (C64, C32) for s in (1, 4, 8) for pc in (False, True)])
HARDER = [("cd24x22", dt, s, False) for dt in (F64, C64) for s in (2, 4, 8)]
SHAPES = [("cd96x90", F64, 4, False), ("cd31x29", F64, 4, False)]


def margin(its):
    return max(5, its // 4)
