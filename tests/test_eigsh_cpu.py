"""The thick-restart Lanczos eigensolver without a GPU: the C ABI and the Python mirror exist, and the numpy checker of the
GPU tests (tests/_eigsh_ref.py) is checked independently of the library — its Ritz pairs against numpy.linalg.eigvalsh of the
dense matrix, its Jacobi routine against numpy.linalg.eigh, its invariant-subspace threshold on matrices built to meet it — and
the cycle and product counts the GPU tests quote are recorded here."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eigsh_ref as ref  # noqa: E402
import _kron  # noqa: E402

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
EPS64 = ref.EPS64
NAMES = sorted(["sprs_eigsh_%s_%s" % (f, s) for f in ("create", "solve", "solve_dev") for s in "dzsc"] + ["sprs_eigsh_destroy"])

# (matrix, k, ncv) -> (cycles, matvecs) of the checker as (smallest wide, smallest single, largest wide, largest single), wide =
# f64 / c64 at tol 1e-10 and single = f32 / c32 at tol 1e-4, the default start vector.  test_counts_and_eigenpairs holds them.
COUNTS = {
    ("poisson12x11x10", 4, 24): ((8, 136), (5, 88), (7, 120), (5, 88)),
    ("poisson12x11x10", 8, 20): ((45, 196), (26, 120), (48, 208), (30, 136)),
    ("poisson12x11x10", 1, 3): ((166, 333), (46, 93), (190, 381), (70, 141)),
    ("poisson12x11x10", 3, 9): ((142, 291), (68, 143), (109, 225), (49, 105)),
    ("poisson12x11x10", 6, 64): ((3, 168), (2, 116), (3, 168), (2, 116)),
    ("symband1500", 4, 24): ((11, 184), (7, 120), (6, 104), (4, 72)),
    ("symband1500", 8, 20): ((107, 444), (51, 220), (33, 148), (18, 88)),
    ("symband1500", 1, 3): ((342, 685), (100, 201), (40, 81), (14, 29)),
    ("symband1500", 3, 9): ((205, 417), (44, 95), (79, 165), (42, 91)),
    ("symband1500", 6, 64): ((4, 220), (3, 168), (2, 116), (2, 116)),
    ("hermband700", 4, 24): ((7, 120), (4, 72), (7, 120), (4, 72)),
    ("hermband700", 8, 20): ((56, 240), (35, 156), (52, 224), (31, 140)),
    ("hermband700", 1, 3): ((81, 163), (25, 51), (494, 989), (152, 305)),
    ("hermband700", 3, 9): ((87, 181), (37, 81), (86, 179), (31, 69)),
    ("hermband700", 6, 64): ((3, 168), (2, 116), (3, 168), (2, 116)),
    ("chgrid9x8", 4, 24): ((3, 56), (2, 40), (3, 56), (2, 40)),
    ("chgrid9x8", 8, 20): ((14, 72), (8, 48), (14, 72), (9, 52)),
    ("chgrid9x8", 1, 3): ((73, 147), (25, 51), (72, 145), (26, 53)),
    ("chgrid9x8", 3, 9): ((39, 85), (19, 45), (37, 81), (18, 43)),
    ("chgrid9x8", 6, 64): ((1, 64), (1, 64), (1, 64), (1, 64)),
}
MATRICES = ("poisson12x11x10", "symband1500", "hermband700", "chgrid9x8")
KM = ((4, 24), (8, 20), (1, 3), (3, 9), (6, 64))
WHICH = ("smallest", "largest")


def is_single(dt):
    return np.dtype(dt) in (np.dtype(F32), np.dtype(C32))


def dtypes_of(name):
    return (C64, C32) if name in ("hermband700", "chgrid9x8") else (F64, F32)


def count(name, k, m, which, dt):
    return COUNTS[(name, k, m)][2 * WHICH.index(which) + (1 if is_single(dt) else 0)]


@functools.lru_cache(maxsize=None)
def _arrays(name):
    from sprsolve_amd import gen
    if name == "poisson12x11x10":
        ip, ix, d = gen.poisson3d(12, 11, 10)[:3]
    elif name == "poisson8x8x8":
        ip, ix, d = gen.poisson3d(8, 8, 8)[:3]
    elif name == "symband1500":
        ip, ix, d = gen.symmetric_banded(1500)[:3]
    elif name == "symband30":
        ip, ix, d = gen.symmetric_banded(30)[:3]
    elif name == "hermband700":
        ip, ix, d = gen.hermitian_banded(700)[:3]
    elif name == "chgrid9x8":
        ip, ix, d = gen.complex_hermitian_grid(9, 8)[:3]
    elif name == "diag40":
        ip, ix, d = np.arange(41, dtype=np.int32), np.arange(40, dtype=np.int32), np.arange(1.0, 41.0)
    else:
        raise KeyError(name)
    ip, ix, d = np.ascontiguousarray(ip, np.int32), np.ascontiguousarray(ix, np.int32), np.asarray(d)
    for a in (ip, ix, d):
        a.setflags(write=False)
    return ip, ix, d


def system(name, dt):
    """-> (indptr, indices, data in dt)."""
    ip, ix, d = _arrays(name)
    return ip, ix, d.astype(dt)


@functools.lru_cache(maxsize=None)
def spectrum(name):
    """-> (the dense matrix in double, its eigenvalues ascending, |A|_2)."""
    ip, ix, d = _arrays(name)
    A = ref.dense(ip, ix, d.astype(C64 if d.dtype.kind == "c" else F64))
    assert np.array_equal(A, A.conj().T)
    lam = np.linalg.eigvalsh(A)
    A.setflags(write=False); lam.setflags(write=False)
    return A, lam, float(np.max(np.abs(lam)))


def wanted(lam, k, which):
    return lam[:k] if which == "smallest" else lam[::-1][:k]


def true_residual(A, vals, X):
    Xw = X.astype(C64 if X.dtype.kind == "c" else A.dtype)  # (a real matrix run in a complex type has complex vectors)
    return max(float(np.linalg.norm(A @ Xw[i] - float(vals[i]) * Xw[i])) for i in range(len(vals)))


def orth_defect(X):
    Xw = X.astype(C64)
    return float(np.max(np.abs(Xw.conj() @ Xw.T - np.eye(Xw.shape[0]))))


@functools.lru_cache(maxsize=None)
def checker(name, k, m, which, dtname, max_restarts=5000):
    """The restatement's result on the default start vector at the default tolerance (shared, read-only)."""
    dt = np.dtype(dtname).type
    ip, ix, d = system(name, dt)
    o = ref.eigsh(ip, ix, d, k, ref.SMALLEST if which == "smallest" else ref.LARGEST, ref.default_v0(ip.size - 1, dt), m, max_restarts,
                  ref.default_tol(dt), keep_T=True)
    if o.X is not None:
        o.X.setflags(write=False)
    return o


@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_eigsh_abi_and_binding_exist(L):
    src = open(os.path.join(ROOT, "include", "sprsolve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sprs_[a-z0-9_]+)\s*\(", src)) if n.startswith("sprs_eigsh_"))
    assert declared == NAMES
    assert re.search(r"typedef\s+struct\s+sprs_eigsh\s+sprs_eigsh\s*;", src)
    assert re.search(r"SPRS_EIGSH_LARGEST\s*=\s*0\s*,\s*SPRS_EIGSH_SMALLEST\s*=\s*1\b", src)
    assert re.search(r"#define\s+SPRS_EIGSH_MAX_NCV\s+64\b", src)
    for name in NAMES:
        assert hasattr(L, name), name
    out = C.c_void_p()
    for s in "dzsc":
        assert getattr(L, "sprs_eigsh_create_" + s)(None, 4, 0, C.byref(out)) == 7 and not out.value       # a null A
        for f in ("solve", "solve_dev"):
            assert getattr(L, "sprs_eigsh_%s_%s" % (f, s))(None, 1, 0, None, 4, 1, 1e-8, None, None, 0, None, None, None, None) == 7
    assert L.sprs_eigsh_destroy(None) == 0
    import sprsolve_amd
    from sprsolve_amd import _lib
    assert sprsolve_amd.Eigsh.NAME == "eigsh" and _lib.EIGSH_MAX_NCV == ref.MAX_NCV == 64
    assert (_lib.EIGSH_LARGEST, _lib.EIGSH_SMALLEST) == (ref.LARGEST, ref.SMALLEST) == (0, 1)
    assert callable(sprsolve_amd.Eigsh.solve) and callable(sprsolve_amd.Eigsh.new)


def test_round_robin_pairs_meet_once_a_sweep():
    for M in (2, 4, 10, 34, 64):
        seen = set()
        for r in range(M - 1):
            p, q = ref.pairs(r, M)
            assert p.size == M // 2 and np.all(p < q) and sorted(np.concatenate([p, q])) == list(range(M))
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == M * (M - 1) // 2


CASES = [(name, k, m, which, dt) for name in MATRICES for (k, m) in KM for which in WHICH for dt in dtypes_of(name)]
_id = lambda c: "%s-k%d-m%d-%s-%s" % (c[0], c[1], c[2], c[3], np.dtype(c[4]).name)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_counts_and_eigenpairs(case):
    """The restatement converges in the recorded number of cycles and products, to eigenpairs of the dense matrix: every
    |theta_i - lambda_i| <= tol |A|_2 and every true residual <= 2 tol |A|_2 (the estimate equals the true residual up to
    O(m eps |A|), and tol is more than 25 m eps), with orthonormal vectors."""
    name, k, m, which, dt = case
    A, lam, nrm = spectrum(name)
    o = checker(name, k, m, which, np.dtype(dt).name)
    tol = ref.default_tol(dt)
    assert o.status == ref.OK and o.nconv == k
    assert (o.restarts, o.matvecs) == count(name, k, m, which, dt)
    p = ref.restart_size(k, m)
    assert o.matvecs == m + (o.restarts - 1) * (m - p)
    assert o.sweeps <= ref.MAX_SWEEPS
    assert np.max(np.abs(o.vals - wanted(lam, k, which))) <= tol * nrm
    assert true_residual(A, o.vals, o.X) <= 2 * tol * nrm
    assert np.all(o.res <= tol * nrm * (1 + 1e-12))
    # every restart replaces the kept vectors by m-term sums V S (S orthogonal to m eps): up to m eps of orthogonality is lost
    # per cycle and CGS2 restores it for the new vectors only, so the defect may grow like cycles * m * eps
    assert orth_defect(o.X) <= 4 * m * (o.restarts + 1) * float(np.finfo(ref.real_dtype(dt)).eps)


# ---------------------------------------------------------------------------------------------- several tiles a workgroup
# kron_sum(40, n2) (tests/_kron.py), k = 4, ncv = 64, at the least n = 40 n2 that gives every workgroup of the in-place basis
# rotation three tiles and leaves a partial last one on a device of 256 CUs (tests/test_gpu_eigsh.py derives n2 from the device it
# runs on and compares with the restatement at that size): dtype -> (which, n2, cycles, matvecs) of the checker.  One end a
# type; the GPU tests check the other end against the factors' spectra alone.
KRON_N1, KRON_K, KRON_NCV = 40, 4, 64
KRON_COUNTS = {
    "float64": ("smallest", 4916, 5, 288),
    "complex128": ("largest", 2458, 5, 288),
    "float32": ("largest", 9831, 2, 120),
    "complex64": ("smallest", 4916, 3, 176),
}


def kron_n2(num_cu, dt, ncv, k):
    """The least n2 with more than three tiles for every workgroup of the restart's rotation (me = ncv, q = restart_size) and
    of the final one (q = k), and a partial last tile."""
    dt = np.dtype(dt)
    rb = ref.real_dtype(dt).itemsize
    grid = max(_kron.rotate_grid(num_cu, ncv, q, rb)[0] for q in (ref.restart_size(k, ncv), k))
    return _kron.n2_for_tiles(KRON_N1, _kron.TILE_ROWS[dt.name], 3 * grid), grid


@functools.lru_cache(maxsize=None)
def kron_checker(n2, k, m, which, dtname):
    """The restatement on kron_sum(40, n2), the default start vector and tolerance (shared, read-only)."""
    dt = np.dtype(dtname).type
    ip, ix, d, _, _ = _kron.kron_sum(KRON_N1, n2, dt)
    o = ref.eigsh(ip, ix, d, k, ref.SMALLEST if which == "smallest" else ref.LARGEST, ref.default_v0(ip.size - 1, dt), m, 100, ref.default_tol(dt))
    if o.X is not None:
        o.X.setflags(write=False)
    return o


@pytest.mark.parametrize("dtname", sorted(KRON_COUNTS))
def test_kron_counts_and_eigenpairs(dtname):
    """The recorded sizes are the rule's at 256 CUs, and the restatement finds the four extreme pairs of the factors' spectra
    there in the recorded cycles, to the bounds of test_counts_and_eigenpairs."""
    which, n2, cycles, matvecs = KRON_COUNTS[dtname]
    dt = np.dtype(dtname).type
    assert kron_n2(256, dt, KRON_NCV, KRON_K)[0] == n2
    ip, ix, d, lam, nrm = _kron.kron_sum(KRON_N1, n2, dt)
    o = kron_checker(n2, KRON_K, KRON_NCV, which, dtname)
    tol = ref.default_tol(dt)
    assert o.status == ref.OK and o.nconv == KRON_K and (o.restarts, o.matvecs) == (cycles, matvecs)
    assert o.matvecs == KRON_NCV + (o.restarts - 1) * (KRON_NCV - ref.restart_size(KRON_K, KRON_NCV))
    err = float(np.max(np.abs(o.vals - wanted(lam, KRON_K, which))))
    tr = _kron.true_residual(_kron.csr_double(ip, ix, d), o.vals, o.X)
    print("kron40x%d %s %s: |theta - lambda| %.3e (bound %.3e), true residual %.3e (bound %.3e)" % (n2, dtname, which, err, tol * nrm, tr, 2 * tol * nrm))
    assert err <= tol * nrm and tr <= 2 * tol * nrm
    assert orth_defect(o.X) <= 4 * KRON_NCV * (o.restarts + 1) * float(np.finfo(ref.real_dtype(dt)).eps)


def _jacobi_check(T):
    m = T.shape[0]
    theta, S, sweeps, conv = ref.jacobi_eigh(T)
    assert conv and sweeps <= ref.MAX_SWEEPS
    w, _ = np.linalg.eigh(T)
    nrm = max(float(np.max(np.abs(w))), 1e-300)
    bound = 8 * m * EPS64 * nrm
    assert np.max(np.abs(S.T @ T @ S - np.diag(theta))) <= bound
    assert np.max(np.abs(S.T @ S - np.eye(m))) <= 8 * m * EPS64
    assert np.max(np.abs(np.sort(theta) - w)) <= bound
    return sweeps


def _arrowhead(m, scale, seed):
    """diag(theta_0 .. theta_{p-1}) with an arrow row of couplings `scale` g_i at p, tridiagonal from there on: what a restart
    leaves behind.  |T| >= 1."""
    rng = np.random.default_rng(seed)
    p = min(max(m // 3, 0), m - 1) if m > 2 else 0
    T = np.zeros((m, m))
    T[np.arange(m), np.arange(m)] = rng.uniform(-4.0, 4.0, m)
    T[0, 0] = 4.5
    if p > 0:
        g = scale * rng.uniform(-1.0, 1.0, p)
        T[p, :p] = g; T[:p, p] = g
    for j in range(p, m - 1):
        T[j + 1, j] = T[j, j + 1] = rng.uniform(0.1, 1.5) * (scale if j % 3 == 0 else 1.0)
    return T


@pytest.mark.parametrize("m", [2, 3, 9, 20, 33, 64])
@pytest.mark.parametrize("scale", [1.0, 1e-4, 1e-8])
def test_jacobi_on_arrowhead_plus_tridiagonal(m, scale):
    _jacobi_check(_arrowhead(m, scale, 1000 * m + int(-np.log10(scale))))


def test_jacobi_on_the_projected_matrices_of_the_runs():
    most = 0
    for name, k, m, which, dt in [("poisson12x11x10", 4, 24, "smallest", F64), ("symband1500", 8, 20, "largest", F64),
                                  ("hermband700", 6, 64, "smallest", C64), ("chgrid9x8", 3, 9, "largest", C32),
                                  ("poisson12x11x10", 1, 3, "largest", F32), ("chgrid9x8", 6, 64, "smallest", C64)]:
        o = checker(name, k, m, which, np.dtype(dt).name)
        assert len(o.Ts) == o.restarts
        for T in o.Ts[:: max(1, len(o.Ts) // 12)]:
            assert T.shape == (m, m) and np.array_equal(T, T.T)
            most = max(most, _jacobi_check(T))
    assert 1 <= most <= ref.MAX_SWEEPS


def test_jacobi_trivial_sizes():
    theta, S, sweeps, conv = ref.jacobi_eigh(np.array([[3.0]]))
    assert conv and sweeps == 0 and theta[0] == 3.0 and S[0, 0] == 1.0
    theta, S, sweeps, conv = ref.jacobi_eigh(np.diag([2.0, -1.0, 5.0]))
    assert conv and sweeps == 0 and np.array_equal(theta, [2.0, -1.0, 5.0]) and np.array_equal(S, np.eye(3))
    theta, S, sweeps, conv = ref.jacobi_eigh(np.full((3, 3), np.nan))
    assert not conv and sweeps == ref.MAX_SWEEPS             # the cap is reported, never a silent result


@pytest.mark.parametrize("dt", [F64, F32, C64, C32], ids=lambda d: np.dtype(d).name)
def test_invariant_subspace_threshold_on_a_diagonal(dt):
    """diag(1 .. 40), v0 = e5 + e17 (zero-based: the entries 6 and 18): the second step's beta is rounding noise (about 2e-31 in
    f64, 1.6e-13 in f32), under 64 eps scale."""
    ip, ix, d = system("diag40", dt)
    v0 = np.zeros(40, dt); v0[5] = v0[17] = 1
    for which, want in ((ref.LARGEST, [18.0, 6.0]), (ref.SMALLEST, [6.0, 18.0])):
        o = ref.eigsh(ip, ix, d, 2, which, v0, 0, 10, ref.default_tol(dt))
        assert o.status == ref.OK and o.nconv == 2 and o.matvecs == 2 and o.restarts == 1
        assert np.allclose(o.vals, want, rtol=8 * float(np.finfo(ref.real_dtype(dt)).eps), atol=0)
        assert np.all(np.isfinite(o.X)) and np.all(np.isfinite(o.res))
        assert np.all(o.res <= 64 * float(np.finfo(ref.real_dtype(dt)).eps) * 18.0)
        support = np.abs(o.X) > 1e-3
        assert np.array_equal(np.flatnonzero(support.any(axis=0)), [5, 17])
    assert ref.eigsh(ip, ix, d, 3, ref.LARGEST, v0, 0, 10, ref.default_tol(dt)).status == ref.BREAKDOWN
    e5 = np.zeros(40, dt); e5[5] = 1
    o = ref.eigsh(ip, ix, d, 1, ref.SMALLEST, e5, 0, 10, ref.default_tol(dt))
    assert o.status == ref.OK and o.matvecs == 1 and o.vals[0] == 6.0
    o = ref.eigsh(ip, ix, d, 1, ref.SMALLEST, np.zeros(40, dt), 0, 10, ref.default_tol(dt))
    assert o.status == ref.BREAKDOWN and o.matvecs == 0 and o.restarts == 0


@pytest.mark.parametrize("dt", [F64, F32], ids=lambda d: np.dtype(d).name)
def test_invariant_subspace_threshold_on_a_block_diagonal(dt):
    """A 5 + 35 block-diagonal matrix and a start vector in the first block: the fifth step meets the invariant subspace, and the
    pairs are that block's extreme ones, not A's."""
    import scipy.sparse as sp
    rng = np.random.default_rng(7)
    B5 = rng.uniform(-1, 1, (5, 5)); B5 = B5 + B5.T + np.diag(np.arange(5.0))
    B35 = rng.uniform(-1, 1, (35, 35)); B35 = B35 + B35.T + 20 * np.eye(35)
    M = sp.block_diag([B5, B35]).tocsr(); M.sort_indices()
    ip, ix, d = M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(dt)
    v0 = np.zeros(40, dt); v0[:5] = [1.0, -0.5, 0.25, 2.0, 1.5]
    lam5 = np.linalg.eigvalsh(B5)
    eps = float(np.finfo(dt).eps)
    for which, want in ((ref.LARGEST, lam5[::-1][:3]), (ref.SMALLEST, lam5[:3])):
        o = ref.eigsh(ip, ix, d, 3, which, v0, 12, 10, ref.default_tol(dt))
        assert o.status == ref.OK and o.nconv == 3 and o.matvecs == 5 and o.restarts == 1
        assert np.max(np.abs(o.vals - want)) <= 64 * eps * np.max(np.abs(lam5))
        assert np.max(np.abs(o.X[:, 5:])) == 0.0
    assert ref.eigsh(ip, ix, d, 6, ref.LARGEST, v0, 12, 10, ref.default_tol(dt)).status == ref.BREAKDOWN


def test_insufficient_restarts_returns_the_current_pairs():
    ip, ix, d = system("symband1500", F64)
    o = ref.eigsh(ip, ix, d, 3, ref.SMALLEST, ref.default_v0(1500, F64), 9, 1, 1e-10)
    assert o.status == ref.INSUFFICIENT_ITER and o.nconv < 3 and o.restarts == 1 and o.matvecs == 9
    assert np.all(np.isfinite(o.vals)) and np.all(np.isfinite(o.X)) and o.X.shape == (3, 1500)
