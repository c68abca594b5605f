"""The truncated SVD solver without a GPU: the C ABI and the Python mirror exist, and the numpy checker of the GPU tests
(tests/_svds_ref.py) is checked independently of the library — its triplets against numpy.linalg.svd of the dense matrix and
scipy.sparse.linalg.svds, its one-sided Jacobi against numpy.linalg.svd, its invariant-subspace rule on a matrix built to meet
it — and the cycle and product counts the GPU tests quote are recorded here."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lsmr_ref  # noqa: E402
import _svds_ref as ref  # noqa: E402

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
EPS64 = ref.EPS64
NAMES = sorted(["sprs_svds_%s_%s" % (f, s) for f in ("create", "solve", "solve_dev") for s in "dzsc"] + ["sprs_svds_destroy"])

# (matrix, k, ncv, end) -> (cycles, products) of the checker per scalar type, in the order of dtypes_of(matrix) (f64, f32 and,
# for the lsmr* matrices, c64, c32): f64 / c64 at tol 1e-10 and f32 / c32 at tol 1e-4, the default start vector.
# test_counts_and_triplets holds them.  Left out, as the plain Ritz restart converges slowly or not at all at the small end of a
# graded spectrum: (1, 3) smallest on lsmr600x400 (f64: not within 400 cycles), every smallest case but (6, 64) on convdiff30x25
# ((8, 20) and (1, 3): not within 400 cycles), the smallest end of graded1500x700 and poisson12x11x10, (1, 3) on convdiff30x25
# (368 cycles in f64).
COUNTS = {
    ("lsmr130x67", 4, 24, "largest"): ((3, 112), (2, 80), (3, 112), (2, 80)),
    ("lsmr130x67", 4, 24, "smallest"): ((4, 144), (2, 80), (3, 112), (2, 80)),
    ("lsmr130x67", 8, 20, "largest"): ((18, 176), (11, 120), (16, 160), (11, 120)),
    ("lsmr130x67", 8, 20, "smallest"): ((16, 160), (10, 112), (17, 168), (10, 112)),
    ("lsmr130x67", 6, 64, "largest"): ((1, 128), (1, 128), (1, 128), (1, 128)),
    ("lsmr130x67", 6, 64, "smallest"): ((1, 128), (1, 128), (1, 128), (1, 128)),
    ("lsmr130x67", 1, 3, "largest"): ((63, 254), (23, 94), (53, 214), (18, 74)),
    ("lsmr130x67", 1, 3, "smallest"): ((62, 250), (23, 94), (87, 350), (31, 126)),
    ("lsmr67x130", 4, 24, "largest"): ((3, 112), (1, 48), (2, 80), (2, 80)),
    ("lsmr67x130", 4, 24, "smallest"): ((4, 144), (3, 112), (4, 144), (3, 112)),
    ("lsmr67x130", 8, 20, "largest"): ((17, 168), (13, 136), (13, 136), (8, 96)),
    ("lsmr67x130", 8, 20, "smallest"): ((19, 184), (11, 120), (19, 184), (12, 128)),
    ("lsmr67x130", 6, 64, "largest"): ((1, 128), (1, 128), (1, 128), (1, 128)),
    ("lsmr67x130", 6, 64, "smallest"): ((1, 128), (1, 128), (1, 128), (1, 128)),
    ("lsmr67x130", 1, 3, "largest"): ((36, 146), (14, 58), (191, 766), (59, 238)),
    ("lsmr67x130", 1, 3, "smallest"): ((52, 210), (17, 70), (58, 234), (22, 90)),
    ("lsmr600x400", 4, 24, "largest"): ((5, 176), (3, 112), (5, 176), (3, 112)),
    ("lsmr600x400", 4, 24, "smallest"): ((10, 336), (6, 208), (9, 304), (6, 208)),
    ("lsmr600x400", 8, 20, "largest"): ((31, 280), (20, 192), (31, 280), (20, 192)),
    ("lsmr600x400", 8, 20, "smallest"): ((74, 624), (50, 432), (67, 568), (41, 360)),
    ("lsmr600x400", 6, 64, "largest"): ((2, 232), (2, 232), (2, 232), (2, 232)),
    ("lsmr600x400", 6, 64, "smallest"): ((3, 336), (2, 232), (3, 336), (2, 232)),
    ("lsmr600x400", 1, 3, "largest"): ((55, 222), (18, 74), (215, 862), (54, 218)),
    ("convdiff30x25", 4, 24, "largest"): ((9, 304), (5, 176)),
    ("convdiff30x25", 8, 20, "largest"): ((40, 352), (25, 232)),
    ("convdiff30x25", 6, 64, "largest"): ((3, 336), (2, 232)),
    ("convdiff30x25", 6, 64, "smallest"): ((14, 1480), (10, 1064)),
    ("graded1500x700", 4, 24, "largest"): ((4, 144), (3, 112)),
    ("graded1500x700", 8, 20, "largest"): ((20, 192), (14, 144)),
    ("graded1500x700", 6, 64, "largest"): ((2, 232), (1, 128)),
    ("graded1500x700", 1, 3, "largest"): ((33, 134), (14, 58)),
    ("poisson12x11x10", 4, 24, "largest"): ((5, 176), (3, 112)),
    ("poisson12x11x10", 8, 20, "largest"): ((29, 264), (19, 184)),
    ("poisson12x11x10", 6, 64, "largest"): ((2, 232), (2, 232)),
    ("poisson12x11x10", 1, 3, "largest"): ((95, 382), (32, 130)),
}


def dtypes_of(name):
    return (F64, F32, C64, C32) if name.startswith("lsmr") else (F64, F32)


def count(name, k, m, which, dt):
    return COUNTS[(name, k, m, which)][[np.dtype(d) for d in dtypes_of(name)].index(np.dtype(dt))]


@functools.lru_cache(maxsize=None)
def _arrays(name):
    """-> (shape, indptr, indices, data in the widest type the matrix is used in)."""
    from sprsolve_amd import gen
    if name.startswith("lsmr"):
        r, c = (int(v) for v in name[4:].split("x"))
        ip, ix, d = _lsmr_ref.system(r, c, C64, seed=r + c)[:3]          # (the real types take the real part)
        shape = (r, c)
    elif name == "convdiff30x25":
        ip, ix, d = gen.convection_diffusion_2d(30, 25)[:3]
        shape = (750, 750)
    elif name == "graded1500x700":
        ip, ix, d = _lsmr_ref.system(1500, 700, F64, seed=2200)[:3]
        d = d * (1.0 + 9.0 * (ix / 699.0) ** 4)                         # column j scaled by 1 + 9 (j / (n - 1))^4
        shape = (1500, 700)
    elif name == "poisson12x11x10":
        ip, ix, d = gen.poisson3d(12, 11, 10)[:3]
        shape = (1320, 1320)
    elif name == "lsmr30x20":
        ip, ix, d = _lsmr_ref.system(30, 20, C64, seed=50)[:3]
        shape = (30, 20)
    elif name == "diag50x40":
        ip = np.minimum(np.arange(51), 40); ix = np.arange(40); d = np.arange(1.0, 41.0)     # A[i, i] = i + 1, ten empty rows
        shape = (50, 40)
    else:
        raise KeyError(name)
    ip, ix, d = np.ascontiguousarray(ip, np.int32), np.ascontiguousarray(ix, np.int32), np.asarray(d)
    for a in (ip, ix, d):
        a.setflags(write=False)
    return shape, ip, ix, d


def system(name, dt):
    """-> (shape, indptr, indices, data in dt)."""
    shape, ip, ix, d = _arrays(name)
    return shape, ip, ix, (d if np.dtype(dt).kind == "c" else d.real).astype(dt)


@functools.lru_cache(maxsize=None)
def spectrum(name, complex_):
    """-> (the dense matrix in double, its singular values descending)."""
    shape, ip, ix, d = system(name, C64 if complex_ else F64)
    A = ref.dense(shape, ip, ix, d)
    sv = np.linalg.svd(A, compute_uv=False)
    A.setflags(write=False); sv.setflags(write=False)
    return A, sv


def spectrum_of(name, dt):
    return spectrum(name, np.dtype(dt).kind == "c")


def wanted(sv, k, which):
    return sv[::-1][:k] if which == "smallest" else sv[:k]


def true_residuals(A, s, U, V):
    """max |A v_i - s_i u_i| and max |A^H u_i - s_i v_i|, formed in double."""
    Uw, Vw = U.astype(A.dtype), V.astype(A.dtype)
    AH = A.conj().T
    return (max(float(np.linalg.norm(A @ Vw[i] - float(s[i]) * Uw[i])) for i in range(len(s))),
            max(float(np.linalg.norm(AH @ Uw[i] - float(s[i]) * Vw[i])) for i in range(len(s))))


def orth_defect(X):
    Xw = X.astype(C64)
    return float(np.max(np.abs(Xw.conj() @ Xw.T - np.eye(Xw.shape[0]))))


@functools.lru_cache(maxsize=None)
def checker(name, k, m, which, dtname, max_restarts=400):
    """The restatement's result on the default start vector at the default tolerance (shared, read-only)."""
    dt = np.dtype(dtname).type
    shape, ip, ix, d = system(name, dt)
    o = ref.svds(shape, ip, ix, d, k, ref.SMALLEST if which == "smallest" else ref.LARGEST, ref.default_v0(shape, dt), m, max_restarts,
                 ref.default_tol(dt), keep_B=True)
    for a in (o.U, o.V):
        if a is not None:
            a.setflags(write=False)
    return o


@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_svds_abi_and_binding_exist(L):
    src = open(os.path.join(ROOT, "include", "sprsolve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sprs_[a-z0-9_]+)\s*\(", src)) if n.startswith("sprs_svds_"))
    assert declared == NAMES
    assert re.search(r"typedef\s+struct\s+sprs_svds\s+sprs_svds\s*;", src)
    assert re.search(r"SPRS_SVDS_LARGEST\s*=\s*0\s*,\s*SPRS_SVDS_SMALLEST\s*=\s*1\b", src)
    assert re.search(r"#define\s+SPRS_SVDS_MAX_NCV\s+64\b", src)
    from sprsolve_amd import _lib
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in _lib.PROTOTYPES, name
    out = C.c_void_p()
    for s in "dzsc":
        assert getattr(L, "sprs_svds_create_" + s)(None, None, 0, C.byref(out)) == 7 and not out.value       # a null A
        for f in ("solve", "solve_dev"):
            assert getattr(L, "sprs_svds_%s_%s" % (f, s))(None, 1, 0, None, 4, 1, 1e-8, None, None, 0, None, 0, None, None, None, None) == 7
    assert L.sprs_svds_destroy(None) == 0
    import sprsolve_amd
    assert sprsolve_amd.Svds.NAME == "svds" and _lib.SVDS_MAX_NCV == ref.MAX_NCV == 64
    assert (_lib.SVDS_LARGEST, _lib.SVDS_SMALLEST) == (ref.LARGEST, ref.SMALLEST) == (0, 1)
    assert callable(sprsolve_amd.Svds.solve) and callable(sprsolve_amd.Svds.new)


CASES = [(name, k, m, which, dt) for (name, k, m, which) in COUNTS for dt in dtypes_of(name)]
_id = lambda c: "%s-k%d-m%d-%s-%s" % (c[0], c[1], c[2], c[3], np.dtype(c[4]).name)


def test_the_cases_are_the_listed_ones():
    km = {(4, 24), (8, 20), (6, 64), (1, 3)}
    for name in ("lsmr130x67", "lsmr67x130", "lsmr600x400"):
        for which in ("largest", "smallest"):
            have = {(k, m) for (n_, k, m, w) in COUNTS if n_ == name and w == which}
            assert have == (km - {(1, 3)} if (name, which) == ("lsmr600x400", "smallest") else km)
    assert {(k, m, w) for (n_, k, m, w) in COUNTS if n_ == "convdiff30x25"} == {(4, 24, "largest"), (8, 20, "largest"), (6, 64, "largest"),
                                                                              (6, 64, "smallest")}
    assert {(k, m, w) for (n_, k, m, w) in COUNTS if n_ == "graded1500x700"} == {(k, m, "largest") for (k, m) in km}
    assert all(c[0] <= 220 for v in COUNTS.values() for c in v)
    A, sv = spectrum("convdiff30x25", False)
    assert 1.4e2 < sv[0] / sv[-1] < 1.6e2 and not np.array_equal(A, A.T)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_counts_and_triplets(case):
    """The restatement converges in the recorded number of cycles and products, to singular triplets of the dense matrix: every
    |sigma_i - sigma_i(dense)| <= tol |A|_2 and both true residuals <= 2 tol |A|_2 (the estimate equals the true residual up to
    O(m eps |A|), and tol is more than 25 m eps), with orthonormal vectors."""
    name, k, m, which, dt = case
    A, sv = spectrum_of(name, dt)
    nrm = float(sv[0])
    o = checker(name, k, m, which, np.dtype(dt).name)
    tol = ref.default_tol(dt)
    assert o.status == ref.OK and o.nconv == k
    assert (o.restarts, o.matvecs) == count(name, k, m, which, dt)
    p = ref.restart_size(k, m)
    assert o.matvecs == 2 * m + 2 * (m - p) * (o.restarts - 1)
    assert o.sweeps <= ref.MAX_SWEEPS
    assert o.U.shape == (k, A.shape[0]) and o.V.shape == (k, A.shape[1])
    assert np.max(np.abs(o.s - wanted(sv, k, which))) <= tol * nrm
    r1, r2 = true_residuals(A, o.s, o.U, o.V)
    assert r1 <= 2 * tol * nrm and r2 <= 2 * tol * nrm
    assert np.all(o.res <= tol * nrm * (1 + 1e-12))
    # every restart replaces the kept vectors by m-term sums P Y, Q X (X, Y orthogonal to m eps): up to m eps of orthogonality is
    # lost per cycle and CGS2 restores it for the new vectors only, so the defect may grow like cycles * m * eps
    bound = 4 * m * (o.restarts + 1) * float(np.finfo(ref.real_dtype(dt)).eps)
    assert orth_defect(o.U) <= bound and orth_defect(o.V) <= bound


@pytest.mark.parametrize("name,k,m,dt", [("lsmr600x400", 4, 24, F64), ("graded1500x700", 8, 20, F64)], ids=str)
def test_largest_triplets_against_scipy_svds(name, k, m, dt):
    import scipy.sparse.linalg as spla
    shape, ip, ix, d = system(name, dt)
    o = checker(name, k, m, "largest", np.dtype(dt).name)
    u, s, vt = spla.svds(ref.matrix(shape, ip, ix, d), k=k, which="LM", tol=1e-12)
    srt = np.argsort(-s)
    s, u, vt = s[srt], u[:, srt], vt[srt]
    nrm = float(spectrum_of(name, dt)[1][0])
    assert np.max(np.abs(o.s - s)) <= ref.default_tol(dt) * nrm
    for i in range(k):          # the same vectors up to a common sign (the gaps of these spectra are far above tol)
        sg = np.sign(np.vdot(u[:, i], o.U[i]).real)
        assert np.linalg.norm(o.U[i] - sg * u[:, i]) <= 1e-6 and np.linalg.norm(o.V[i] - sg * vt[i]) <= 1e-6


# ---------------------------------------------------------------------------------------------- the one-sided Jacobi
MOST_SWEEPS = 10     # the most sweeps any matrix of this file takes (asserted below; DESIGN 4n quotes it)


def _jacobi_check(B):
    """-> sweeps.  The relative error of every sigma_i, |X^T B Y - Sigma| / |B|_2 and the two orthogonality defects, all under
    8 m eps."""
    m = B.shape[0]
    sigma, X, Y, sweeps, conv = ref.jacobi_svd(B)
    assert conv and sweeps <= ref.MAX_SWEEPS
    sv = np.linalg.svd(B, compute_uv=False)
    bound = 8 * m * EPS64
    rel = np.max(np.abs(np.sort(sigma)[::-1] - sv) / sv)
    resid = np.max(np.abs(X.T @ B @ Y - np.diag(sigma))) / sv[0]
    ox, oy = np.max(np.abs(X.T @ X - np.eye(m))), np.max(np.abs(Y.T @ Y - np.eye(m)))
    print("m = %d: %d sweeps, relative sigma error %.2e, |X^T B Y - Sigma| / |B| %.2e, defects %.2e %.2e (bound %.2e)" % (m, sweeps, rel, resid, ox, oy, bound))
    assert rel <= bound and resid <= bound and ox <= bound and oy <= bound
    return sweeps


def _spiked(m, scale, seed):
    """diag(sigma_0 .. sigma_{p-1}) with a spike column of couplings `scale` g_i at p, upper bidiagonal from there on: what a
    restart leaves behind and the steps after it add.  |B| >= 1."""
    rng = np.random.default_rng(seed)
    p = min(max(m // 3, 0), m - 1) if m > 2 else 0
    B = np.zeros((m, m))
    B[np.arange(m), np.arange(m)] = rng.uniform(0.5, 4.0, m)
    B[0, 0] = 4.5
    if p > 0:
        B[:p, p] = scale * rng.uniform(-1.0, 1.0, p)
    for j in range(p, m - 1):
        B[j, j + 1] = rng.uniform(0.1, 1.5) * (scale if j % 3 == 0 else 1.0)
    return B


@pytest.mark.parametrize("m", [3, 9, 20, 64])
@pytest.mark.parametrize("scale", [1.0, 1e-4, 1e-8])
def test_jacobi_on_diagonal_plus_spike_plus_bidiagonal(m, scale):
    assert _jacobi_check(_spiked(m, scale, 1000 * m + int(-np.log10(scale)))) <= MOST_SWEEPS


def test_jacobi_on_the_projected_matrices_of_the_runs():
    most = 0
    for name, k, m, which, dt in [("lsmr130x67", 4, 24, "smallest", F64), ("lsmr600x400", 8, 20, "largest", F64),
                                  ("lsmr67x130", 6, 64, "smallest", C64), ("lsmr130x67", 1, 3, "largest", C32),
                                  ("convdiff30x25", 6, 64, "smallest", F64), ("graded1500x700", 6, 64, "largest", F32)]:
        o = checker(name, k, m, which, np.dtype(dt).name)
        assert len(o.Bs) == o.restarts
        for B in o.Bs[:: max(1, len(o.Bs) // 12)]:
            assert B.shape == (m, m) and np.array_equal(B, np.triu(B))
            most = max(most, _jacobi_check(B))
    print("the most sweeps on the projected matrices of the runs: %d" % most)
    assert 1 <= most <= MOST_SWEEPS <= ref.MAX_SWEEPS


def test_every_case_stays_under_the_quoted_sweeps():
    assert max(checker(*c[:4], np.dtype(c[4]).name).sweeps for c in CASES) <= MOST_SWEEPS


def test_jacobi_trivial_sizes():
    sigma, X, Y, sweeps, conv = ref.jacobi_svd(np.array([[3.0]]))
    assert conv and sweeps == 0 and sigma[0] == 3.0 and X[0, 0] == 1.0 and Y[0, 0] == 1.0
    sigma, X, Y, sweeps, conv = ref.jacobi_svd(np.diag([2.0, 1.0, 5.0]))
    assert conv and sweeps == 0 and np.array_equal(sigma, [2.0, 1.0, 5.0]) and np.array_equal(X, np.eye(3)) and np.array_equal(Y, np.eye(3))
    assert not ref.jacobi_svd(np.full((3, 3), np.nan))[4]              # never a silent result
    assert not ref.jacobi_svd(np.diag([2.0, 0.0, 5.0]))[4]             # a zero singular value is reported


# ---------------------------------------------------------------------------------------------- the events
@pytest.mark.parametrize("dt", [F64, F32, C64, C32], ids=lambda d: np.dtype(d).name)
def test_invariant_subspace_on_a_rectangular_diagonal(dt):
    """50 x 40 with A[i, i] = i + 1, v0 = e5 + e17 (zero-based: the entries 6 and 18): the second step's beta is rounding noise,
    under 64 eps scale — four products."""
    shape, ip, ix, d = system("diag50x40", dt)
    v0 = np.zeros(40, dt); v0[5] = v0[17] = 1
    eps = float(np.finfo(ref.real_dtype(dt)).eps)
    for which, want in ((ref.LARGEST, [18.0, 6.0]), (ref.SMALLEST, [6.0, 18.0])):
        o = ref.svds(shape, ip, ix, d, 2, which, v0, 0, 10, ref.default_tol(dt))
        assert o.status == ref.OK and o.nconv == 2 and o.matvecs == 4 and o.restarts == 1
        assert np.allclose(o.s, want, rtol=8 * eps, atol=0)
        assert np.all(o.res == 0.0) and np.all(np.isfinite(o.U)) and np.all(np.isfinite(o.V))
        assert o.U.shape == (2, 50) and o.V.shape == (2, 40)
        for Z in (o.U, o.V):
            assert np.array_equal(np.flatnonzero((np.abs(Z) > 1e-3).any(axis=0)), [5, 17])
    assert ref.svds(shape, ip, ix, d, 3, ref.LARGEST, v0, 0, 10, ref.default_tol(dt)).status == ref.BREAKDOWN
    o = ref.svds(shape, ip, ix, d, 1, ref.SMALLEST, np.zeros(40, dt), 0, 10, ref.default_tol(dt))
    assert o.status == ref.BREAKDOWN and o.matvecs == 0 and o.restarts == 0


def test_the_swap_puts_the_start_vector_in_the_small_space():
    shape, ip, ix, d = system("lsmr67x130", F64)
    assert ref.default_v0(shape, F64).size == 67 == ref.default_v0((130, 67), F64).size
    o = checker("lsmr67x130", 4, 24, "largest", "float64")
    assert o.U.shape == (4, 67) and o.V.shape == (4, 130)


def test_insufficient_restarts_returns_the_current_triplets():
    shape, ip, ix, d = system("lsmr600x400", F64)
    o = ref.svds(shape, ip, ix, d, 3, ref.SMALLEST, ref.default_v0(shape, F64), 9, 1, 1e-10)
    assert o.status == ref.INSUFFICIENT_ITER and o.nconv < 3 and o.restarts == 1 and o.matvecs == 18
    assert np.all(np.isfinite(o.s)) and np.all(np.isfinite(o.U)) and np.all(np.isfinite(o.V))
    assert o.U.shape == (3, 600) and o.V.shape == (3, 400)
