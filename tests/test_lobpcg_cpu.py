"""The LOBPCG eigensolver without a GPU: the C ABI and the Python mirror exist, and the numpy checker of the GPU tests
(tests/_lobpcg_ref.py) is checked independently of the library — its pairs against numpy.linalg.eigvalsh of the dense matrix,
its Hermitian Jacobi routine against numpy.linalg.eigh, its [X, W] fallback on a basis built to need it, the 6 b <= n rule, its
soft locking and stopping threshold on matrices with isolated extreme eigenvalues (tests/_kron.py) — and the iteration counts
that cap the GPU runs are recorded here."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kron  # noqa: E402
import _lobpcg_ref as ref  # noqa: E402
from test_eigsh_cpu import orth_defect, spectrum, system, true_residual, wanted  # noqa: E402

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
EPS64 = ref.EPS64
NAMES = sorted(["sprs_lobpcg_%s_%s" % (f, s) for f in ("create", "solve", "solve_dev") for s in "dzsc"]
               + ["sprs_%s_lobpcg_solve_dev_%s" % (p, s) for p in ("ilu0", "amg", "fsai") for s in "dzsc"] + ["sprs_lobpcg_destroy"])

# (matrix, k, b) -> (iters, restarts) of the checker, `which` major ("smallest", "largest") and the matrix's dtypes minor, no
# preconditioner, the default start block, tol 1e-10 (f64 / c64) and 1e-4 (f32 / c32).  test_counts_and_eigenpairs holds them.
# (Regenerated when anorm became a Rayleigh quotient of held vectors and locked columns left the projected problem: anorm is
# never larger than the largest Ritz value it replaced, so most counts rose by one or two iterations.)
COUNTS = {
    ("poisson12x11x10", 4, 8): ((67, 0), (30, 1), (65, 0), (28, 1)),
    ("poisson12x11x10", 3, 5): ((83, 0), (34, 0), (81, 0), (31, 0)),
    ("poisson12x11x10", 1, 1): ((169, 0), (66, 0), (94, 0), (36, 0)),
    ("symband1500", 4, 8): ((115, 0), (42, 2), (47, 0), (20, 1)),
    ("symband1500", 3, 5): ((129, 0), (46, 1), (60, 0), (26, 1)),
    ("symband1500", 1, 1): ((156, 0), (60, 0), (42, 0), (18, 0)),
    ("hermband700", 4, 8): ((64, 0), (26, 1), (61, 0), (24, 0)),
    ("hermband700", 3, 5): ((72, 0), (29, 1), (67, 0), (27, 0)),
    ("hermband700", 1, 1): ((69, 0), (29, 0), (101, 0), (35, 0)),
    ("chgrid9x8", 4, 8): ((26, 0), (12, 1), (27, 0), (12, 0)),
    ("chgrid9x8", 3, 5): ((37, 0), (16, 0), (36, 0), (16, 0)),
    ("chgrid9x8", 1, 1): ((64, 0), (27, 0), (49, 0), (22, 0)),
    ("symband30", 3, 5): ((28, 0), (12, 1), (30, 0), (12, 0), (19, 0), (8, 0), (20, 0), (9, 0)),
    ("symband30", 2, 3): ((36, 0), (15, 1), (37, 0), (15, 0), (28, 0), (11, 0), (30, 0), (13, 0)),
    ("poisson8x8x8", 4, 8): ((49, 0), (48, 0)),
}
MATRICES = ("poisson12x11x10", "symband1500", "hermband700", "chgrid9x8")
KB = ((4, 8), (3, 5), (1, 1))
WHICH = ("smallest", "largest")


def is_single(dt):
    return np.dtype(dt) in (np.dtype(F32), np.dtype(C32))


def dtypes_of(name):
    if name == "symband30":
        return (F64, F32, C64, C32)
    if name == "poisson8x8x8":
        return (F64,)
    return (C64, C32) if name in ("hermband700", "chgrid9x8") else (F64, F32)


def count(name, k, b, which, dt):
    dts = [np.dtype(d) for d in dtypes_of(name)]
    return COUNTS[(name, k, b)][len(dts) * WHICH.index(which) + dts.index(np.dtype(dt))]


@functools.lru_cache(maxsize=None)
def checker(name, k, b, which, dtname, max_iter=5000):
    """The restatement's result on the default start block at the default tolerance, no preconditioner (shared, read-only)."""
    dt = np.dtype(dtname).type
    ip, ix, d = system(name, dt)
    o = ref.lobpcg(ip, ix, d, k, ref.SMALLEST if which == "smallest" else ref.LARGEST, ref.default_X0(ip.size - 1, b, dt), max_iter,
                   ref.default_tol(dt))
    if o.X is not None:
        o.X.setflags(write=False)
    return o


@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_lobpcg_abi_and_binding_exist(L):
    src = open(os.path.join(ROOT, "include", "sprsolve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sprs_[a-z0-9_]+)\s*\(", src)) if "lobpcg" in n)
    assert declared == NAMES
    assert re.search(r"typedef\s+struct\s+sprs_lobpcg\s+sprs_lobpcg\s*;", src)
    assert re.search(r"#define\s+SPRS_LOBPCG_MAX_BLOCK\s+8\b", src)
    for name in NAMES:
        assert hasattr(L, name), name
    out = C.c_void_p()
    for s in "dzsc":
        assert getattr(L, "sprs_lobpcg_create_" + s)(None, 48, 0, C.byref(out)) == 7 and not out.value       # a null A
        for f in ("lobpcg_solve", "lobpcg_solve_dev", "ilu0_lobpcg_solve_dev", "amg_lobpcg_solve_dev", "fsai_lobpcg_solve_dev"):
            assert getattr(L, "sprs_%s_%s" % (f, s))(None, None, 1, 1, None, 0, 1, 1e-8, None, None, 0, None, None, None, None, None) == 7
    assert L.sprs_lobpcg_destroy(None) == 0
    import sprsolve_amd
    from sprsolve_amd import _lib
    assert sprsolve_amd.Lobpcg.NAME == "lobpcg" and _lib.LOBPCG_MAX_BLOCK == ref.MAX_BLOCK == 8
    assert callable(sprsolve_amd.Lobpcg.solve) and callable(sprsolve_amd.Lobpcg.new) and callable(sprsolve_amd.Lobpcg.default_X0)


def test_python_mirror_validates_its_arguments(L):
    import sprsolve_amd as sa

    class FakeA:
        dtype = np.dtype(F64)
    with pytest.raises(ValueError, match="block"):
        sa.Lobpcg.new(FakeA(), 48, -1)
    S = sa.Lobpcg.__new__(sa.Lobpcg)
    S.A, S.size, S.dtype, S.s, S.h, S.block = FakeA(), 48, np.dtype(F64), "d", None, 8
    with pytest.raises(ValueError, match="which"):
        S.solve(2, which="both")
    with pytest.raises(TypeError, match="precond"):
        S.solve(2, precond=object())
    X0 = S.default_X0()
    assert X0.shape == (8, 48) and X0.dtype == F64 and np.array_equal(X0, ref.default_X0(48, 8, F64))
    S.dtype, S.s = np.dtype(C32), "c"
    assert np.array_equal(S.default_X0(), ref.default_X0(48, 8, C32)) and S.default_X0().dtype == C32


def test_block_rule():
    """6 b <= n and b <= 8: with b = 8 on n = 30 the [X, W] basis of 16 vectors goes rank-deficient within three iterations."""
    assert ref.block_ok(5, 30) and not ref.block_ok(6, 30) and not ref.block_ok(8, 30) and not ref.block_ok(9, 1500) and not ref.block_ok(0, 30)
    assert ref.default_block(30) == 5 and ref.default_block(1500) == 8 and ref.default_block(6) == 1
    ip, ix, d = system("symband30", F64)
    with pytest.raises(AssertionError):
        ref.lobpcg(ip, ix, d, 4, ref.SMALLEST, ref.default_X0(30, 8, F64), 10, 1e-10)


CASES = [(name, k, b, which, dt) for name in MATRICES for (k, b) in KB for which in WHICH for dt in dtypes_of(name)]
EDGE_CASES = [("symband30", k, b, which, dt) for (k, b) in ((3, 5), (2, 3)) for which in WHICH for dt in dtypes_of("symband30")]
MULT_CASES = [("poisson8x8x8", 4, 8, which, F64) for which in WHICH]
_id = lambda c: "%s-k%d-b%d-%s-%s" % (c[0], c[1], c[2], c[3], np.dtype(c[4]).name)


@pytest.mark.parametrize("case", CASES + EDGE_CASES + MULT_CASES, ids=_id)
def test_counts_and_eigenpairs(case):
    """The restatement converges in the recorded number of iterations and fallbacks, to eigenpairs of the dense matrix: every
    |theta_i - lambda_i| <= tol |A|_2 and every true residual <= 2 tol |A|_2 (the stopping rule bounds the computed residual by
    tol anorm <= tol |A|_2; the factor 2 is Eigsh's allowance for forming it again in double), multiple eigenvalues with their
    multiplicity."""
    name, k, b, which, dt = case
    A, lam, nrm = spectrum(name)
    o = checker(name, k, b, which, np.dtype(dt).name)
    tol = ref.default_tol(dt)
    assert o.status == ref.OK and o.nconv == k
    assert (o.iters, o.restarts) == count(name, k, b, which, dt)
    assert o.matvecs == b * (o.iters + 1)
    assert o.sweeps <= ref.MAX_SWEEPS
    assert np.max(np.abs(o.vals - wanted(lam, k, which))) <= tol * nrm
    assert true_residual(A, o.vals, o.X) <= 2 * tol * nrm
    assert np.all(o.res <= tol * nrm * (1 + 1e-12))
    # X = S C with C from a Cholesky-orthonormalised problem: the defect is the Gram sums' rounding, about m eps
    assert orth_defect(o.X) <= 64 * float(np.finfo(ref.real_dtype(dt)).eps)


def test_multiple_eigenvalues_are_found_with_multiplicity():
    """poisson3d(8, 8, 8): the second smallest (and second largest) eigenvalue is triple; a block of 8 finds all copies."""
    A, lam, nrm = spectrum("poisson8x8x8")
    assert abs(lam[1] - lam[3]) <= 1e-12 * nrm and lam[1] - lam[0] > 1e-3 * nrm
    for which in WHICH:
        o = checker("poisson8x8x8", 4, 8, which, "float64")
        assert np.max(np.abs(o.vals - wanted(lam, 4, which))) <= 1e-10 * nrm


# ---------------------------------------------------------------------------------------------- isolated extreme eigenvalues
# A = I (x) T1 + T2 (x) I (tests/_kron.py), n = 40 n2: four isolated eigenvalues at each end (about +-4.0, 3.5, 3.2, 3.0) over a
# cluster.  The leading columns converge tens of iterations before the others; before soft locking their W_c (rounding noise) and
# P_c stayed in the basis, G went singular to working precision while still passing the Cholesky rule, the projected problem
# returned Ritz values of 1e11 .. 1e27, anorm took them and the solve ended SPRS_OK with residuals of 1e-2 (c64) or in a
# breakdown.  Truth is the factors' spectra; the start block is the default or a fixed normal one.
KRON_N1 = 40
KRON_MAX_ITER = 400
KRON_CASES = [(50, which, dt, x0) for dt in (F64, F32, C64, C32) for which in WHICH for x0 in ("default", "normal")] \
    + [(100, "smallest", C64, "default"), (400, "smallest", C64, "default")]
_kron_id = lambda c: "kron40x%d-%s-%s-%s" % (c[0], c[1], np.dtype(c[2]).name, c[3])


def kron_X0(n, b, dt, kind):
    """The default start block, or standard normal entries from default_rng(5) (the real parts first, then the imaginary)."""
    if kind == "default":
        return ref.default_X0(n, b, dt)
    rng = np.random.default_rng(5)
    X0 = rng.standard_normal((b, n))
    if np.dtype(dt).kind == "c":
        X0 = X0 + 1j * rng.standard_normal((b, n))
    return X0.astype(dt)


@functools.lru_cache(maxsize=None)
def kron_checker(n2, which, dtname, x0, k=4, b=8):
    """The restatement's result on kron_sum(40, n2) at the default tolerance, max_iter 400 (shared, read-only)."""
    dt = np.dtype(dtname).type
    ip, ix, d, _, _ = _kron.kron_sum(KRON_N1, n2, dt)
    o = ref.lobpcg(ip, ix, d, k, ref.SMALLEST if which == "smallest" else ref.LARGEST, kron_X0(ip.size - 1, b, dt, x0), KRON_MAX_ITER,
                   ref.default_tol(dt))
    if o.X is not None:
        o.X.setflags(write=False)
    return o


def check_kron_pairs(n2, dt, k, which, status, vals, X, label):
    """A run that says OK holds the bounds of test_counts_and_eigenpairs against the factors' spectra; one that does not converge
    says INSUFFICIENT_ITER, or BREAKDOWN without vectors."""
    ip, ix, d, lam, nrm = _kron.kron_sum(KRON_N1, n2, dt)
    tol = ref.default_tol(dt)
    if status != ref.OK:
        assert status == ref.INSUFFICIENT_ITER or (status == ref.BREAKDOWN and X is None), status
        print("%s: status %d (not converged)" % (label, status))
        return False
    err = float(np.max(np.abs(np.asarray(vals, F64) - wanted(lam, k, which))))
    tr = _kron.true_residual(_kron.csr_double(ip, ix, d), vals, X)
    print("%s: n %d, |theta - lambda| %.3e (bound %.3e), true residual %.3e (bound %.3e)" % (label, ip.size - 1, err, tol * nrm, tr, 2 * tol * nrm))
    assert err <= tol * nrm
    assert tr <= 2 * tol * nrm
    return True


@pytest.mark.parametrize("case", KRON_CASES, ids=_kron_id)
def test_isolated_extreme_eigenvalues(case):
    n2, which, dt, x0 = case
    o = kron_checker(n2, which, np.dtype(dt).name, x0)
    print("iters %d, fallbacks %d, nconv %d, reported residuals %s" % (o.iters, o.restarts, o.nconv, o.res))
    if check_kron_pairs(n2, dt, 4, which, o.status, o.vals, o.X, _kron_id(case)):
        nrm = _kron.kron_sum(KRON_N1, n2, dt)[4]
        assert o.nconv == 4 and np.all(o.res <= ref.default_tol(dt) * nrm * (1 + 1e-12))
        assert orth_defect(o.X) <= 64 * float(np.finfo(ref.real_dtype(dt)).eps)


def test_anorm_never_exceeds_the_norm_and_locked_columns_leave_the_basis():
    """The stopping threshold is tol anorm: anorm is a Rayleigh quotient of held vectors, so at most |A|_2, whatever the projected
    problem returns; and a locked column's P and W rows of C are zero."""
    rng = np.random.default_rng(11)
    n, b = 90, 3
    A = rng.standard_normal((n, n)); A = A + A.T
    S = rng.standard_normal((3 * b, n))
    S[2 * b] = S[0] + 1e-5 * S[2 * b]                          # W_0 all but inside the span of X: an ill-conditioned G that passes
    G, K = S @ S.T, S @ (A @ S.T)
    eps = float(np.finfo(F64).eps)
    nrm = float(np.linalg.norm(A, 2))
    rr = ref.rayleigh_ritz(G, K, b, True, ref.SMALLEST, eps)
    assert rr.ok and 0.0 < rr.anorm <= nrm
    lock = np.array([True, False, False])
    lk = ref.rayleigh_ritz(G, K, b, True, ref.SMALLEST, eps, lock)
    assert lk.ok and lk.C.shape == (3 * b, 3 * b - 2) and np.all(lk.C[b] == 0) and np.all(lk.C[2 * b] == 0) and 0.0 < lk.anorm <= nrm
    free = np.r_[0:b, b + 1:2 * b, 2 * b + 1:3 * b]
    Y = (S[free].T @ lk.C[free]).T
    assert np.max(np.abs(Y @ Y.T - np.eye(3 * b - 2))) <= 1e-10
    assert np.max(np.abs(Y @ (A @ Y.T) - np.diag(lk.theta))) <= 1e-10 * nrm


# ---------------------------------------------------------------------------------------------- the Jacobi routine
def _jacobi_check(K):
    m = K.shape[0]
    theta, Z, sweeps, conv = ref.jacobi_eigh_h(K)
    assert conv and sweeps <= ref.MAX_SWEEPS and theta.dtype == np.float64
    w, _ = np.linalg.eigh(K)
    nrm = max(float(np.max(np.abs(w))), 1e-300)
    bound = 8 * m * EPS64 * nrm
    assert np.max(np.abs(Z.conj().T @ K @ Z - np.diag(theta))) <= bound
    assert np.max(np.abs(Z.conj().T @ Z - np.eye(m))) <= 8 * m * EPS64
    assert np.max(np.abs(np.sort(theta) - w)) <= bound
    return sweeps


@pytest.mark.parametrize("m", [1, 2, 3, 6, 9, 15, 16, 24])
@pytest.mark.parametrize("kind", ["real", "complex"])
@pytest.mark.parametrize("spread", [1.0, 1e-6])
def test_jacobi_against_eigh(m, kind, spread):
    """Dense Hermitian matrices of the sizes the solver meets (m = b, 2 b, 3 b), also with a cluster of eigenvalues."""
    rng = np.random.default_rng(100 * m + (7 if kind == "complex" else 0))
    Q = rng.standard_normal((m, m)) + (1j * rng.standard_normal((m, m)) if kind == "complex" else 0)
    Q, _ = np.linalg.qr(Q)
    lam = np.concatenate([[-3.0], 1.0 + spread * rng.uniform(-1, 1, m - 1)])[:m]
    K = (Q * lam) @ Q.conj().T
    K = (K + K.conj().T) / 2
    _jacobi_check(K)


def test_jacobi_trivial_sizes_and_the_cap():
    theta, Z, sweeps, conv = ref.jacobi_eigh_h(np.array([[3.0]]))
    assert conv and sweeps == 0 and theta[0] == 3.0 and Z[0, 0] == 1.0
    theta, Z, sweeps, conv = ref.jacobi_eigh_h(np.diag([2.0, -1.0, 5.0]).astype(C64))
    assert conv and sweeps == 0 and np.array_equal(theta, [2.0, -1.0, 5.0]) and np.array_equal(Z, np.eye(3))
    theta, Z, sweeps, conv = ref.jacobi_eigh_h(np.full((3, 3), np.nan))
    assert not conv and sweeps == ref.MAX_SWEEPS             # the cap is reported, never a silent result
    K = np.array([[1.0, 2j], [-2j, 1.0]])                    # a purely imaginary pivot: the rotation carries its phase
    theta, Z, sweeps, conv = ref.jacobi_eigh_h(K)
    assert conv and np.allclose(np.sort(theta), [-1.0, 3.0], rtol=0, atol=4 * EPS64)


# ---------------------------------------------------------------------------------------------- the fallback
@pytest.mark.parametrize("kind", ["real", "complex"])
def test_fallback_when_p_lies_in_the_span_of_x_and_w(kind):
    """[X, P, W] with P = X Y + W Z: G is singular, the Cholesky rule fails on the full basis and the step is repeated on
    [X, W] with the P rows of C zero — the same Ritz values as a step that never had P."""
    rng = np.random.default_rng(5 if kind == "real" else 6)
    n, b = 60, 3
    cx = (lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)) if kind == "complex" else (lambda *s: rng.standard_normal(s))
    A = cx(n, n); A = A + A.conj().T
    X, W = cx(b, n), cx(b, n)
    P = (cx(b, b) @ X + cx(b, b) @ W)
    S = np.concatenate([X, P, W]); AS = (A @ S.T).T
    G, K = S.conj() @ S.T, S.conj() @ AS.T
    eps = float(np.finfo(np.float64).eps)
    rr = ref.rayleigh_ritz(G, K, b, True, ref.SMALLEST, eps)
    assert rr.ok and rr.fell_back and not rr.used_p and rr.C.shape == (3 * b, 2 * b) and np.all(rr.C[b:2 * b] == 0)
    no_p = ref.rayleigh_ritz(G, K, b, False, ref.SMALLEST, eps)
    assert no_p.ok and not no_p.fell_back and np.array_equal(no_p.theta, rr.theta) and np.array_equal(no_p.C, rr.C)
    Sxw = np.concatenate([X, W])
    Y = (Sxw.T @ rr.C[np.r_[0:b, 2 * b:3 * b]]).T
    assert np.max(np.abs(Y.conj() @ Y.T - np.eye(2 * b))) <= 1e-10
    assert np.max(np.abs(Y.conj() @ (A @ Y.T) - np.diag(rr.theta))) <= 1e-10 * np.linalg.norm(A, 2)
    # an independent P is used, and a dependent basis without P is a failure
    full = ref.rayleigh_ritz(*(lambda S2: (S2.conj() @ S2.T, S2.conj() @ (A @ S2.T)))(np.concatenate([X, cx(b, n), W])), b, True, ref.SMALLEST, eps)
    assert full.ok and full.used_p and not full.fell_back and full.C.shape == (3 * b, 3 * b)
    S3 = np.concatenate([X, P, X[::-1].copy()])
    bad = ref.rayleigh_ritz(S3.conj() @ S3.T, S3.conj() @ (A @ S3.T), b, True, ref.SMALLEST, eps)
    assert not bad.ok and bad.fell_back


def test_events_of_the_restatement():
    ip, ix, d = system("symband1500", F64)
    X0 = ref.default_X0(1500, 8, F64)
    o = ref.lobpcg(ip, ix, d, 4, ref.SMALLEST, X0, 1, 1e-10)
    assert o.status == ref.INSUFFICIENT_ITER and o.nconv < 4 and o.iters == 1 and o.matvecs == 16
    assert np.all(np.isfinite(o.vals)) and np.all(np.isfinite(o.X)) and o.X.shape == (4, 1500)
    Z = X0.copy(); Z[3] = 0
    o = ref.lobpcg(ip, ix, d, 4, ref.SMALLEST, Z, 10, 1e-10)
    assert o.status == ref.BREAKDOWN and o.matvecs == 8 and o.X is None
    E = X0[:2].copy(); E[1] = E[0]
    o = ref.lobpcg(ip, ix, d, 1, ref.SMALLEST, E, 10, 1e-10)
    assert o.status == ref.BREAKDOWN and o.iters == 0
    bad = d.copy(); bad[3] = np.nan
    assert ref.lobpcg(ip, ix, bad, 4, ref.SMALLEST, X0, 10, 1e-10).status == ref.BREAKDOWN
    # a Jacobi preconditioner (the diagonal of M) leaves the pairs alone
    A, lam, nrm = spectrum("symband1500")
    o = ref.lobpcg(ip, ix, d, 4, ref.SMALLEST, X0, 2000, 1e-10, prec=1.0 / np.diag(A))
    assert o.status == ref.OK and np.max(np.abs(o.vals - lam[:4])) <= 1e-10 * nrm and true_residual(A, o.vals, o.X) <= 2e-10 * nrm
