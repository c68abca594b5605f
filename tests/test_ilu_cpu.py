"""The ILU(0) checker (tests/_ilu_ref.py) checked on the CPU: its factors against a dense LU where ILU(0) is the complete LU,
its level rules against the grids' closed forms, its creation errors, and the iteration counts that tests/test_gpu_ilu.py takes
its max_iter from (at least twice the count, the rule of tests/test_gpu_cg.py).  The systems of the GPU file are built here."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ilu_ref as ref  # noqa: E402

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]


def is_single(dt):
    return np.dtype(dt) in (np.dtype(F32), np.dtype(C32))


def tol_of(dt):
    return 1e-5 if is_single(dt) else 1e-10


# ------------------------------------------------------------------------------------------------ the systems
def cg_system(dt):
    """f64: poisson3d(12, 11, 10).  The other types: a small Hermitian positive-definite case whose ILU(0) drops fill — the
    7-point Poisson matrix on 8 x 7 x 6, for the complex types turned by a diagonal unitary similarity (a_ij e^{i(t_i - t_j)}):
    Hermitian, the same spectrum, complex off-diagonals.  rhs uniform."""
    from sprsolve_amd import gen
    if np.dtype(dt) == np.dtype(F64):
        ip, ix, d, rhs = gen.poisson3d(12, 11, 10)
        return ip, ix, d, rhs
    ip, ix, d, _ = gen.poisson3d(8, 7, 6)
    n = ip.size - 1
    rhs = gen.uniform(gen.SEED, n, stream=81)
    if np.dtype(dt).kind == "c":
        th = gen.uniform(gen.SEED, n, lo=0.0, hi=2 * np.pi, stream=82)
        rows = np.repeat(np.arange(n), np.diff(ip))
        d = d * np.exp(1j * (th[rows] - th[ix]))
        d[rows == ix] = 6.0
        rhs = rhs + 1j * gen.uniform(gen.SEED, n, stream=83)
    return ip, ix, d.astype(dt), rhs.astype(dt)


GMRES_RESTART = 10                                            # at least two cycles: the ILU(0) counts below exceed it

# the checker's counts, x0 = 0, f64 / c64 at tol 1e-10 and f32 / c32 at 1e-5, in the order of ALL: (Jacobi, ILU(0))
CG_COUNTS = {"float64": (44, 21), "complex128": (41, 15), "float32": (23, 8), "complex64": (23, 8)}
GMRES_COUNTS = {"float64": (111, 32), "complex128": (111, 32), "float32": (70, 17), "complex64": (70, 17)}


# Trace rows of the GMRES case compared at rtol 1e-9 / atol 1e-12 (by the self-check below and by the GPU test, both modes): the
# first 20, i.e. the first two cycles.  tests/test_gmres_cpu.py's rule: a restart forms rhs - A x with a relative error of
# eps |rhs| / |r|, which the following cycle's scalars inherit, and ILU(0) brings |r| / |rhs| to 1e-6 within two cycles.  The
# checker against itself with its sums taken pairwise holds a TENTH of that tolerance on rows 1 .. 20 in f64 and c64; the first
# row outside the tenth is row 21 (c64) / 25 (f64), the first outside the tolerance itself row 31 (of 32).
GMRES_TRACE_ROWS = 20


def indefinite_system():
    """A symmetric INDEFINITE matrix whose ILU(0) exists: the 5-point grid operator on 8 x 7 (diag 4, neighbours -1) with the
    diagonal of 10 seeded nodes set to -4.  ILU(0)-CG on it ends in InvalidPreconditioner at iteration 3 with
    re(rho_new) = -1.9e-3, six orders above the rounding of that sum."""
    from sprsolve_amd import gen
    ip, ix, d, _ = gen.convection_diffusion_2d(8, 7, cx=0.0, cy=0.0)
    n = ip.size - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    neg = gen.uniform(2, n, stream=7) > 0.6
    d = d.copy()
    d[(rows == ix) & neg[rows]] = -4.0
    return ip, ix, d, gen.uniform(2, n, stream=8)


def ragged_system(n=1000, seed=0x1107):
    """Seeded, non-symmetric, strictly diagonally dominant, ragged: row i has 1 .. 12 entries (one in twelve rows holds only its
    diagonal), the off-diagonal columns anywhere in the matrix.  Rows of very different lengths share a 64-row slice."""
    from sprsolve_amd import gen
    length = 1 + (gen.splitmix64(seed, n, stream=1) % np.uint64(12)).astype(np.int64)
    R, Cc = [], []
    for i in range(n):
        c = (gen.splitmix64_keys(seed, i * 16 + np.arange(length[i] - 1), stream=2) % np.uint64(n)).astype(np.int64)
        c = np.unique(c[c != i])
        R.append(np.full(c.size + 1, i)); Cc.append(np.concatenate([c, [i]]))
    R = np.concatenate(R); Cc = np.concatenate(Cc)
    order = np.lexsort((Cc, R))
    R, Cc = R[order], Cc[order]
    v = gen.uniform_keys(seed, R * n + Cc, stream=3)
    absrow = np.zeros(n)
    np.add.at(absrow, R[R != Cc], np.abs(v[R != Cc]))
    v[R == Cc] = 1.0 + absrow
    ip = np.zeros(n + 1, np.int64); np.cumsum(np.bincount(R, minlength=n), out=ip[1:])
    return ip.astype(np.int32), Cc.astype(np.int32), v, gen.uniform(seed, n, stream=4)


@functools.lru_cache(maxsize=None)
def factors_of(name, dtname):
    """(ip, ix, d, rhs, checker factors) of a named system, computed once and shared (read-only)."""
    from sprsolve_amd import gen
    dt = np.dtype(dtname).type
    if name == "cd24x20":
        ip, ix, d, rhs = gen.convection_diffusion_2d(24, 20, dtype=dt)
    elif name == "herm300":
        ip, ix, d, rhs = gen.hermitian_banded(300, 3)
    elif name == "p3_64x64x8":
        ip, ix, d, rhs = gen.poisson3d(64, 64, 8)
        rhs = gen.uniform(gen.SEED, rhs.size, stream=84)
    elif name == "tri300":
        ip, ix, d, rhs = gen.random_tridiagonal(300)
    elif name == "ragged1000":
        ip, ix, d, rhs = ragged_system()
    elif name == "cg":
        ip, ix, d, rhs = cg_system(dt)
    elif name == "indefinite":
        ip, ix, d, rhs = indefinite_system()
    else:
        raise KeyError(name)
    d = d.astype(dt); rhs = rhs.astype(dt)
    f = ref.ilu0(ip, ix, d)
    assert f.status == ref.OK, (name, f)
    for a in (ip, ix, d, rhs, f.val):
        a.setflags(write=False)
    return ip, ix, d, rhs, f.val


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.real.dtype.itemsize]) if a.dtype.kind != "c" else a.view(a.real.dtype).view({4: np.uint32, 8: np.uint64}[a.real.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ 1. dense LU
def _dense_lu(M):
    """No-pivot Doolittle LU in place, the k-i-j loop order, every operation rounded once in M's dtype."""
    S = ref.Scalar(M.dtype)
    n = M.shape[0]
    a = [[S.load(v) for v in row] for row in M]
    for k in range(n):
        for i in range(k + 1, n):
            l = S.div(a[i][k], a[k][k])
            a[i][k] = l
            for j in range(k + 1, n):
                a[i][j] = S.sub(a[i][j], S.mul(l, a[k][j]))
    return np.array([[S.store(v) for v in row] for row in a], dtype=M.dtype)


def _banded_csr(M, hbw):
    n = M.shape[0]
    R, Cc = np.nonzero(np.abs(np.subtract.outer(np.arange(n), np.arange(n))) <= hbw)
    ip = np.zeros(n + 1, np.int32); np.cumsum(np.bincount(R, minlength=n), out=ip[1:])
    return ip, Cc.astype(np.int32), M[R, Cc].copy()


@pytest.mark.parametrize("dt", [F64, F32], ids=lambda d: np.dtype(d).name)
def test_factors_equal_a_dense_lu_where_nothing_is_dropped(dt):
    """A tridiagonal matrix, and a 5 x 4 grid stored dense inside its band, have no fill outside their pattern: ILU(0) is the
    complete LU.  Entry (i, j) receives its updates l_ik u_kj for k = 0 .. min(i, j) - 1 in ascending k in the checker's
    row-by-row order and in the dense k-i-j order alike (the dense loop's extra updates subtract a product with an exact zero),
    so the bits agree."""
    from sprsolve_amd import gen
    ip, ix, d, _ = gen.random_tridiagonal(40)
    gp, gx, gd, _ = gen.convection_diffusion_2d(5, 4)
    G = np.zeros((20, 20)); G[np.repeat(np.arange(20), np.diff(gp)), gx] = gd
    bp, bx, bd = _banded_csr(G, 4)
    for name, (p, x, v) in (("tridiagonal", (ip, ix, d)), ("band", (bp, bx, bd))):
        v = v.astype(dt)
        n = p.size - 1
        M = np.zeros((n, n), dt); rows = np.repeat(np.arange(n), np.diff(p)); M[rows, x] = v
        f = ref.ilu0(p, x, v)
        assert f.status == ref.OK
        LU = _dense_lu(M)
        assert np.array_equal(bits(f.val), bits(LU[rows, x])), name
        outside = np.ones((n, n), bool); outside[rows, x] = False
        assert not np.any(LU[outside]), name                 # the dense LU made no fill outside the pattern


# ------------------------------------------------------------------------------------------------ 2. levels
def test_level_counts_of_the_grids():
    from sprsolve_amd import gen
    for rows, cols in ((5, 4), (24, 20), (3, 9)):
        ip, ix, _, _ = gen.convection_diffusion_2d(rows, cols)
        assert ref.level_counts(ip, ix) == (rows + cols - 1, rows + cols - 1)
    for nx, ny, nz in ((12, 11, 10), (5, 3, 4), (64, 64, 8)):
        ip, ix, _, _ = gen.poisson3d(nx, ny, nz)
        assert ref.level_counts(ip, ix) == (nx + ny + nz - 2, nx + ny + nz - 2)
    ip, ix, _, _ = gen.random_tridiagonal(300)
    assert ref.level_counts(ip, ix) == (300, 300)
    lv, ul = ref.levels(*gen.poisson3d(64, 64, 8)[:2])
    assert np.bincount(lv).max() == 496 and 496 % 64 != 0    # levels larger than a 256-thread workgroup, ending in a partial slice


# ------------------------------------------------------------------------------------------------ 3. iteration counts
@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_ilu_cg_needs_fewer_iterations_than_jacobi(dt):
    ip, ix, d, rhs, f = factors_of("cg", np.dtype(dt).name)
    n = rhs.size
    want_j, want_i = CG_COUNTS[np.dtype(dt).name]
    oj = ref.cg(ip, ix, d, rhs, np.zeros(n, dt), 2 * want_j, tol_of(dt), prec=ref.jacobi(ip, ix, d))
    oi = ref.cg(ip, ix, d, rhs, np.zeros(n, dt), 2 * want_i, tol_of(dt), prec=ref.Applier(ip, ix, f))
    print("cg %s: Jacobi %d, ILU(0) %d iterations" % (np.dtype(dt).name, oj.its, oi.its))
    assert (oj.status, oj.its) == (ref.OK, want_j) and (oi.status, oi.its) == (ref.OK, want_i)
    assert oi.its < oj.its and oi.its >= 4                   # (enough iterations for a trace to compare)


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_ilu_gmres_needs_fewer_steps_than_jacobi(dt):
    ip, ix, d, rhs, f = factors_of("cd24x20", np.dtype(dt).name)
    n = rhs.size
    want_j, want_i = GMRES_COUNTS[np.dtype(dt).name]
    oj = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 2 * want_j, tol_of(dt), restart=GMRES_RESTART, prec=ref.jacobi(ip, ix, d))
    oi = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 2 * want_i, tol_of(dt), restart=GMRES_RESTART, prec=ref.Applier(ip, ix, f))
    print("gmres %s: Jacobi %d, ILU(0) %d steps" % (np.dtype(dt).name, oj.its, oi.its))
    assert (oj.status, oj.its) == (ref.OK, want_j) and (oi.status, oi.its) == (ref.OK, want_i)
    assert oi.its < oj.its and oi.its > GMRES_RESTART        # at least two cycles


@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_gmres_checker_holds_the_gpu_tolerances_against_itself(dt):
    """tests/test_gmres_cpu.py::_self_check for the ILU(0) case: with its sums taken pairwise the checker keeps the status, the
    step count, res (rtol 1e-9 / atol 1e-12), x (1e-7 max|x|) and the first GMRES_TRACE_ROWS trace rows — those within a tenth of
    rtol 1e-9 / atol 1e-12, which is how the prefix was chosen."""
    import _gmres_ref
    from test_gmres_cpu import trace_close
    ip, ix, d, rhs, f = factors_of("cd24x20", np.dtype(dt).name)
    n = rhs.size
    want = GMRES_COUNTS[np.dtype(dt).name][1]
    ap = ref.Applier(ip, ix, f)
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 2 * want, 1e-10, restart=GMRES_RESTART, prec=ap)
    p = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 2 * want, 1e-10, restart=GMRES_RESTART, prec=ap, sums="pairwise")
    assert p.status == o.status == ref.OK and p.its == o.its == want
    assert np.isclose(p.res, o.res, rtol=1e-9, atol=1e-12)
    assert np.max(np.abs(p.x - o.x)) <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
    k = GMRES_TRACE_ROWS
    assert 15 <= k <= o.its
    tp, to = _gmres_ref.trace_array(p.trace[:k]), _gmres_ref.trace_array(o.trace[:k])
    assert trace_close(tp, to, rtol=1e-9, atol=1e-12) and trace_close(tp, to, rtol=1e-10, atol=1e-13)


def test_callable_checkers_agree_with_the_diagonal_ones():
    """ref.cg / ref.gmres with the Jacobi callable are tests/_cg_ref.py's and tests/_gmres_ref.py's with precond_diag."""
    import _cg_ref
    import _gmres_ref
    ip, ix, d, rhs, _ = factors_of("cd24x20", "float64")
    dg = d[np.repeat(np.arange(rhs.size), np.diff(ip)) == ix]
    a = ref.gmres(ip, ix, d, rhs, np.zeros(rhs.size), 300, 1e-10, restart=GMRES_RESTART, prec=ref.jacobi(ip, ix, d))
    b = _gmres_ref.gmres(ip, ix, d, rhs, np.zeros(rhs.size), 300, 1e-10, restart=GMRES_RESTART, precond_diag=dg)
    assert (a.status, a.its, a.res) == (b.status, b.its, b.res) and np.array_equal(a.x, b.x)
    ip, ix, d, rhs, _ = factors_of("cg", "float64")
    dg = d[np.repeat(np.arange(rhs.size), np.diff(ip)) == ix]
    a = ref.cg(ip, ix, d, rhs, np.zeros(rhs.size), 100, 1e-10, prec=ref.jacobi(ip, ix, d))
    b = _cg_ref.cg(ip, ix, d, rhs, np.zeros(rhs.size), 100, 1e-10, precond_diag=dg)
    assert (a.status, a.its, a.res) == (b.status, b.its, b.res) and np.array_equal(a.x, b.x)


def test_indefinite_matrix_ends_in_invalid_preconditioner():
    ip, ix, d, rhs, f = factors_of("indefinite", "float64")
    o = ref.cg(ip, ix, d, rhs, np.zeros(rhs.size), 50, 1e-10, prec=ref.Applier(ip, ix, f))
    assert (o.status, o.its) == (ref.INVALID_PRECOND, 3) and -3e-3 < o.res < -1e-3


# ------------------------------------------------------------------------------------------------ 4. creation errors
def test_creation_errors():
    ip = np.array([0, 2, 4], np.int32); ix = np.array([0, 1, 0, 1], np.int32)
    for dt in ALL:
        f = ref.ilu0(ip, ix, np.ones(4, dt))
        assert (f.status, f.row, f.val) == (ref.ZERO_DIAGONAL, 1, None)       # u_11 = 1 - 1*1
    # a missing diagonal reports its (smallest) row
    ip3 = np.array([0, 2, 3, 5, 6], np.int32); ix3 = np.array([0, 1, 0, 1, 2, 2], np.int32)
    f = ref.ilu0(ip3, ix3, np.ones(6))
    assert (f.status, f.row) == (ref.ZERO_DIAGONAL, 1)
    # unsorted and duplicate columns
    assert ref.ilu0(ip, np.array([1, 0, 0, 1], np.int32), np.ones(4))[:2] == (ref.INVALID_ARGUMENT, 0)
    assert ref.ilu0(ip, np.array([0, 1, 1, 1], np.int32), np.ones(4))[:2] == (ref.INVALID_ARGUMENT, 1)
    # a non-finite pivot counts as a zero one; rows downstream simply carry it
    f = ref.ilu0(ip, ix, np.array([np.inf, 1.0, 1.0, 1.0]))
    assert (f.status, f.row) == (ref.ZERO_DIAGONAL, 0)


def test_folds_invert_the_factors():
    """L (L^-1 r) = r and U (U^-1 y) = y to rounding, and which = 0 is the two in sequence, bit for bit."""
    ip, ix, d, rhs, f = factors_of("ragged1000", "float64")
    n = rhs.size
    assert np.diff(ip).min() == 1 and np.diff(ip).max() <= 12
    ap = ref.Applier(ip, ix, f)
    y, z, both = ap.solve(1, rhs), ap.solve(2, rhs), ap.solve(0, rhs)
    assert np.array_equal(bits(ap.solve(2, y)), bits(both))
    import scipy.sparse as sp
    M = sp.csr_matrix((f, ix, ip), shape=(n, n))
    L = sp.tril(M, -1) + sp.identity(n); U = sp.triu(M, 0)
    assert np.max(np.abs(L @ y - rhs)) <= 1e-13 and np.max(np.abs(U @ z - rhs)) <= 1e-13
