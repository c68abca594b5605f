"""The AMG checker (tests/_amg_ref.py) checked on the CPU: its hierarchy against scipy's products, the two conditions the
coarsening rule has to meet, the symmetry of the cycle, its creation errors, and the iteration counts that tests/test_gpu_amg.py
takes its max_iter from (at least twice the count, the rule of tests/test_gpu_cg.py).  The systems of the GPU file are built
here.  Every right-hand side is a seeded uniform vector: the generators' own A.1 lies in the range of every aggregation
prolongator, and AMG-CG would "converge" on it in one iteration."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _amg_ref as amg  # noqa: E402
import _ilu_ref as ref  # noqa: E402
from test_ilu_cpu import ALL, C32, C64, F32, F64, bits, cg_system, ragged_system, tol_of  # noqa: E402,F401

THETA, COARSE_MAX, MAX_LEVELS = 0.08, 256, 16                 # the defaults of AMG.new
RHS_SEED = 7


def _complex_rhs(n, dt):
    from sprsolve_amd import gen
    rhs = gen.uniform(RHS_SEED, n, stream=3)
    if np.dtype(dt).kind == "c":
        rhs = rhs + 1j * gen.uniform(RHS_SEED, n, stream=4)
    return rhs.astype(dt)


def rotate(ip, ix, d, dt, diag):
    """A real symmetric matrix turned by a diagonal unitary similarity (a_ij e^{i(t_i - t_j)}) for the complex types: Hermitian,
    the same spectrum, complex off-diagonals (tests/test_ilu_cpu.py::cg_system's construction)."""
    from sprsolve_amd import gen
    if np.dtype(dt).kind != "c":
        return d.astype(dt)
    n = ip.size - 1
    th = gen.uniform(gen.SEED, n, lo=0.0, hi=2 * np.pi, stream=82)
    rows = np.repeat(np.arange(n), np.diff(ip))
    d = d * np.exp(1j * (th[rows] - th[ix]))
    d[rows == ix] = diag
    return d.astype(dt)


def indefinite_grid():
    """A symmetric INDEFINITE matrix: the 5-point grid operator on 24 x 20 (diag 4, neighbours -1) with the diagonal of the seeded
    nodes set to -4.  (tests/test_ilu_cpu.py::indefinite_system has 56 rows: below coarse_max, where the cycle is an exact LU solve
    and CG converges at once.)  AMG-CG on it ends in InvalidPreconditioner at iteration 4 with re(rho_new) = -2.3e-5, eleven
    orders above the rounding of that sum."""
    from sprsolve_amd import gen
    ip, ix, d, _ = gen.convection_diffusion_2d(24, 20, cx=0.0, cy=0.0)
    n = ip.size - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    neg = gen.uniform(2, n, stream=7) > 0.6
    d = d.copy()
    d[(rows == ix) & neg[rows]] = -4.0
    return ip, ix, d, gen.uniform(2, n, stream=8)


@functools.lru_cache(maxsize=None)
def system_of(name, dtname):
    """(ip, ix, d, rhs) of a named system in a scalar type, computed once and shared (read-only)."""
    from sprsolve_amd import gen
    dt = np.dtype(dtname).type
    if name.startswith("p3_"):
        dims = tuple(int(v) for v in name[3:].split("x"))
        ip, ix, d, _ = gen.poisson3d(*dims)
        d = rotate(ip, ix, d, dt, 6.0)
    elif name == "cd24x20":
        ip, ix, d, _ = gen.convection_diffusion_2d(24, 20, dtype=dt)
    elif name == "cd64x64":
        ip, ix, d, _ = gen.convection_diffusion_2d(64, 64)
    elif name == "tri300":
        ip, ix, d, _ = gen.random_tridiagonal(300)
    elif name == "ragged1000":
        ip, ix, d, _ = ragged_system()
    elif name == "cg":                                       # the systems of the ILU(0) tests (f64: poisson3d(12, 11, 10))
        ip, ix, d, rhs = cg_system(dt)
    elif name == "indefinite":
        ip, ix, d, rhs = indefinite_grid()
    else:
        raise KeyError(name)
    n = ip.size - 1
    if name not in ("indefinite",) and not (name == "cg" and np.dtype(dt) != np.dtype(F64)):
        rhs = _complex_rhs(n, dt)
    d = d.astype(dt); rhs = rhs.astype(dt)
    for a in (ip, ix, d, rhs):
        a.setflags(write=False)
    return ip, ix, d, rhs


@functools.lru_cache(maxsize=None)
def hierarchy_of(name, dtname, coarse_max=COARSE_MAX):
    ip, ix, d, _ = system_of(name, dtname)
    H = amg.build(ip, ix, d, THETA, coarse_max, MAX_LEVELS)
    assert H.status == amg.OK, (name, H.status, H.row)
    return H


# the checker's counts, x0 = 0, f64 / c64 at tol 1e-10 and f32 / c32 at 1e-5, on system "cg": (ILU(0), AMG)
CG_COUNTS = {"float64": (21, 15), "complex128": (15, 22), "float32": (8, 7), "complex64": (8, 13)}
CG_COUNT_24 = 16                                              # AMG-CG, f64, poisson3d(24, 22, 20)
GMRES_RESTART = 10
GMRES_COUNTS = {"float64": (107, 16), "complex128": (130, 16)}   # cd24x20: (Jacobi, AMG) steps of GMRES(10)
INDEFINITE = (4, -2.3e-5)                                     # iteration and re(rho_new) of the InvalidPreconditioner end
# Trace rows of the GMRES case compared at rtol 1e-9 / atol 1e-12 by the GPU test: the first cycle.  The rule of
# tests/test_ilu_cpu.py: the checker against itself with its sums taken pairwise holds a TENTH of that tolerance on rows 1 .. 10
# in f64 and c64; row 11, the first after the restart, is the first outside the tenth.
GMRES_TRACE_ROWS = 10
# what the GPU tests pass for max_iter (at least twice the count: asserted below)
CG_MAX_ITER, GMRES_MAX_ITER = 50, 40


# ------------------------------------------------------------------------------------------------ 1. the hierarchy
def _sp(n, m, t):
    import scipy.sparse as sp
    return sp.csr_matrix((t[2], t[1], t[0]), shape=(n, m))


def _ones(M):
    """The structural pattern with every value 1: products of such matrices cancel nothing (scipy drops exact zeros)."""
    M = M.tocsr().copy(); M.data = np.ones(M.data.size)
    return M


def _same_pattern(M, ip, ix):
    M = M.tocsr(); M.sort_indices()
    return np.array_equal(M.indptr, ip) and np.array_equal(M.indices, ix)


def test_aggregation_of_a_chain():
    """The 1-D Laplacian on 7 nodes: row 0 founds {0, 1}; row 2 has the aggregated neighbour 1 and waits; row 3 founds {2, 3, 4};
    row 5 waits; row 6 founds {5, 6}.  Nothing is left for passes 2 and 3."""
    n = 7
    ip = np.concatenate([[0], np.cumsum([2] + [3] * (n - 2) + [2])])
    ix = np.concatenate([[0, 1]] + [[i - 1, i, i + 1] for i in range(1, n - 1)] + [[n - 2, n - 1]])
    d = np.where(ix == np.repeat(np.arange(n), np.diff(ip)), 2.0, -1.0)
    op = amg.Ops(F64)
    agg, nc = amg.aggregate(op, ip, ix, d, np.full(n, 2.0), THETA)
    assert nc == 3 and agg.tolist() == [0, 0, 1, 1, 1, 2, 2]
    # weak couplings only (theta = 0.6 > 1/2): every row founds its singleton in pass 1
    agg, nc = amg.aggregate(op, ip, ix, d, np.full(n, 2.0), 0.6)
    assert nc == n and agg.tolist() == list(range(n))


def _graph(n, edges, diag=4.0):
    """CSR arrays of the symmetric matrix with `diag` on the diagonal and the weighted edges {(i, j): a_ij = a_ji}."""
    M = np.zeros((n, n)); M[np.arange(n), np.arange(n)] = diag
    for (i, j), v in edges.items():
        M[i, j] = M[j, i] = v
    R, Cc = np.nonzero(M)
    ip = np.zeros(n + 1, np.int64); np.cumsum(np.bincount(R, minlength=n), out=ip[1:])
    return ip, Cc, M[R, Cc]


def test_aggregation_pass_two_by_hand():
    """Seven nodes, every stored coupling strong (1 >= 0.08^2 * 16).  Pass 1: row 0 founds {0, 1}, row 2 founds {2, 3}; rows 4, 5
    and 6 each have an aggregated neighbour and wait.  Pass 2, on the snapshot taken after pass 1:
      row 4 sees 1 (aggregate 0, |a|^2 = 1) and 3 (aggregate 1, |a|^2 = 1): a tie, the first wins -> 0 (row 6 is not counted);
      row 5 sees 1 (|a|^2 = 1) and 3 (|a|^2 = 4): the largest wins -> 1;
      row 6 sees 3 (|a|^2 = 1) and 4 (|a|^2 = 9), but 4 is unaggregated IN THE SNAPSHOT and does not count -> 1 (reading the
      live array instead would send row 6 after row 4 into aggregate 0)."""
    ip, ix, d = _graph(7, {(0, 1): -1, (2, 3): -1, (1, 4): -1, (3, 4): -1, (1, 5): -1, (3, 5): -2, (3, 6): -1, (4, 6): -3})
    agg, nc = amg.aggregate(amg.Ops(F64), ip, ix, d, np.full(7, 4.0), THETA)
    assert nc == 2 and agg.tolist() == [0, 0, 1, 1, 0, 1, 1]


@pytest.mark.parametrize("name", ["ragged1000", "cd24x20", "tri300", "p3_12x11x10"])
def test_pass_three_has_nothing_left_to_do(name):
    """A row is left over by pass 1 only because one of its strong neighbours was aggregated when it was visited; that neighbour
    is aggregated in the snapshot, so pass 2 places the row.  Pass 3 of the stated rules therefore never founds an aggregate,
    whatever the matrix (strength need not be symmetric: the ragged system): the first two passes leave no row unplaced."""
    ip, ix, d, _ = system_of(name, "float64")
    n = ip.size - 1
    diag = d[np.repeat(np.arange(n), np.diff(ip)) == ix]
    two, nc2 = amg.aggregate(amg.Ops(F64), ip, ix, d, diag, THETA, passes=2)
    three, nc3 = amg.aggregate(amg.Ops(F64), ip, ix, d, diag, THETA)
    assert two.min() >= 0 and nc2 == nc3 and np.array_equal(two, three)
    if name == "ragged1000":
        assert np.any(np.bincount(three) == 1)               # rows without a strong neighbour: singletons of pass 1


@pytest.mark.parametrize("name,dt", [("p3_12x11x10", F64), ("p3_24x22x20", F64), ("cd24x20", F64), ("ragged1000", F64), ("p3_8x7x6", C64),
                                     ("tri300", F32)],
                         ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_hierarchy_against_scipy_products(name, dt):
    """Every level: P = T - omega D^-1 A T, R = P^H and A_c = R A P formed by scipy from the checker's aggregates agree with the
    checker's folds to 1e-12 (f32: 1e-5) of the largest entry, with the same stored pattern."""
    import scipy.sparse as sp
    H = hierarchy_of(name, np.dtype(dt).name)
    tol = 1e-5 if np.dtype(dt) == np.dtype(F32) else 1e-12
    assert len(H.levels) >= 2
    for l, L in enumerate(H.levels[:-1]):
        nc = H.levels[l + 1].n
        assert L.agg.min() == 0 and np.array_equal(np.unique(L.agg), np.arange(nc))       # every aggregate is inhabited
        A = _sp(L.n, L.n, (L.ip, L.ix, L.val)).astype(np.complex128 if np.dtype(dt).kind == "c" else np.float64)
        T = sp.csr_matrix((np.ones(L.n), L.agg, np.arange(L.n + 1)), shape=(L.n, nc))
        Dinv = sp.diags(1.0 / A.diagonal())
        P = T - float(L.omega) * (Dinv @ A @ T)
        mine = _sp(L.n, nc, L.P)
        assert _same_pattern(_ones(A) @ T, L.P[0], L.P[1])
        assert abs(mine - P).max() <= tol * abs(P).max()
        R = _sp(nc, L.n, L.R)
        assert abs(R - mine.conj().T).max() == 0
        Ac = P.conj().T @ A @ P
        C = H.levels[l + 1]
        assert _same_pattern(_ones(R) @ (_ones(A) @ _ones(mine)), C.ip, C.ix)
        assert abs(_sp(nc, nc, (C.ip, C.ix, C.val)) - Ac).max() <= tol * abs(Ac).max()
    if H.lu is not None:
        C = H.levels[-1]
        M = _sp(C.n, C.n, (C.ip, C.ix, C.val)).toarray()
        Lm = np.tril(H.lu, -1) + np.eye(C.n); U = np.triu(H.lu)
        assert np.max(np.abs(Lm @ U - M)) <= tol * np.max(np.abs(M))


@pytest.mark.parametrize("name", ["p3_12x11x10", "p3_24x22x20", "p3_64x64x8", "cd64x64"])
def test_coarsening_reaches_coarse_max_within_twice_the_fine_nnz(name):
    """theta_l = theta 2^-l: the hierarchy ends at <= coarse_max rows through the LU (the half-rows stop never fires), and
    sum_l nnz(A_l) <= 2 nnz(A_0)."""
    H = hierarchy_of(name, "float64")
    rows = [L.n for L in H.levels]; nnz = [int(L.ip[-1]) for L in H.levels]
    print(name, "rows", rows, "nnz", nnz, "sum / nnz0 = %.3f" % (sum(nnz) / nnz[0]))
    assert rows[-1] <= COARSE_MAX and H.lu is not None and len(rows) < MAX_LEVELS
    assert all(2 * b <= a for a, b in zip(rows, rows[1:]))
    assert sum(nnz) <= 2 * nnz[0]


def test_level_sizes_recorded_in_the_design_notes():
    assert [L.n for L in hierarchy_of("p3_12x11x10", "float64").levels] == [1320, 167]
    assert [L.n for L in hierarchy_of("p3_24x22x20", "float64").levels] == [10560, 1293, 138]
    assert [L.n for L in hierarchy_of("p3_64x64x8", "float64").levels] == [32768, 4133, 445, 34]
    assert [L.n for L in hierarchy_of("cd64x64", "float64").levels] == [4096, 704, 102]


def test_half_rows_stop_and_jacobi_coarse_solve():
    """Weak couplings only (theta = 0.6 on the 1-D Laplacian): every row is a singleton, the half-rows stop makes level 0 the
    coarsest, and the cycle is the eight Jacobi sweeps."""
    ip, ix, d, rhs = system_of("tri300", "float64")
    H = amg.build(ip, ix, d, 10.0, 16, MAX_LEVELS)
    assert H.status == amg.OK and len(H.levels) == 1 and H.lu is None
    x = amg.Applier(H)(rhs)
    op = amg.Ops(F64); L = H.levels[0]
    y = rhs * L.omega / L.diag
    for _ in range(amg.COARSE_SWEEPS - 1):
        y = y + (rhs - amg.spmv(op, L.ip, L.ix, L.val, y)) * L.omega / L.diag
    assert np.array_equal(bits(x), bits(y))


# ------------------------------------------------------------------------------------------------ 2. the cycle
@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_cycle_is_hermitian(dt):
    ip, ix, d, _ = system_of("p3_8x7x6", np.dtype(dt).name)
    H = hierarchy_of("p3_8x7x6", np.dtype(dt).name)
    assert len(H.levels) == 2
    ap = amg.Applier(H)
    n = ip.size - 1
    M = np.array([ap(e) for e in np.eye(n, dtype=dt)]).T
    assert np.max(np.abs(M - M.conj().T)) <= 1e-15 * n * np.max(np.abs(M))
    assert np.linalg.eigvalsh((M + M.conj().T) / 2).min() > 0


# ------------------------------------------------------------------------------------------------ 3. iteration counts
@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_amg_cg_counts(dt):
    name = np.dtype(dt).name
    ip, ix, d, rhs = system_of("cg", name)
    n = rhs.size
    want_i, want_a = CG_COUNTS[name]
    f = ref.ilu0(ip, ix, d)
    oi = ref.cg(ip, ix, d, rhs, np.zeros(n, dt), 2 * want_i, tol_of(dt), prec=ref.Applier(ip, ix, f.val))
    oa = ref.cg(ip, ix, d, rhs, np.zeros(n, dt), 2 * want_a, tol_of(dt), prec=amg.Applier(hierarchy_of("cg", name)))
    print("cg %s: ILU(0) %d, AMG %d iterations" % (name, oi.its, oa.its))
    assert (oi.status, oi.its) == (ref.OK, want_i) and (oa.status, oa.its) == (ref.OK, want_a)
    assert oa.its >= 4 and CG_MAX_ITER >= 2 * want_a
    if np.dtype(dt) == np.dtype(F64):
        assert oa.its < oi.its                               # poisson3d(12, 11, 10): fewer than ILU(0) on the same right-hand side


def test_amg_cg_count_is_flat_in_the_grid():
    ip, ix, d, rhs = system_of("p3_24x22x20", "float64")
    o = ref.cg(ip, ix, d, rhs, np.zeros(rhs.size), 2 * CG_COUNT_24, 1e-10, prec=amg.Applier(hierarchy_of("p3_24x22x20", "float64")))
    assert (o.status, o.its) == (ref.OK, CG_COUNT_24)
    assert abs(o.its - CG_COUNTS["float64"][1]) <= 3


@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_amg_gmres_needs_fewer_steps_than_jacobi(dt):
    name = np.dtype(dt).name
    ip, ix, d, rhs = system_of("cd24x20", name)
    n = rhs.size
    want_j, want_a = GMRES_COUNTS[name]
    oj = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 2 * want_j, 1e-10, restart=GMRES_RESTART, prec=ref.jacobi(ip, ix, d))
    oa = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 2 * want_a, 1e-10, restart=GMRES_RESTART, prec=amg.Applier(hierarchy_of("cd24x20", name)))
    assert (oj.status, oj.its) == (ref.OK, want_j) and (oa.status, oa.its) == (ref.OK, want_a)
    assert GMRES_RESTART < oa.its < oj.its and GMRES_MAX_ITER >= 2 * want_a


@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_gmres_checker_holds_the_gpu_tolerances_against_itself(dt):
    """tests/test_ilu_cpu.py's self-check for the AMG case: with its sums taken pairwise the checker keeps the status, the step
    count, res, x and the first GMRES_TRACE_ROWS trace rows within a tenth of rtol 1e-9 / atol 1e-12; the next row is outside."""
    import _gmres_ref
    from test_gmres_cpu import trace_close
    name = np.dtype(dt).name
    ip, ix, d, rhs = system_of("cd24x20", name)
    n = rhs.size
    want = GMRES_COUNTS[name][1]
    ap = amg.Applier(hierarchy_of("cd24x20", name))
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 2 * want, 1e-10, restart=GMRES_RESTART, prec=ap)
    p = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 2 * want, 1e-10, restart=GMRES_RESTART, prec=ap, sums="pairwise")
    assert p.status == o.status == ref.OK and p.its == o.its == want
    assert np.isclose(p.res, o.res, rtol=1e-9, atol=1e-12)
    assert np.max(np.abs(p.x - o.x)) <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
    k = GMRES_TRACE_ROWS
    tp, to = _gmres_ref.trace_array(p.trace[:k]), _gmres_ref.trace_array(o.trace[:k])
    assert trace_close(tp, to, rtol=1e-10, atol=1e-13)
    tp, to = _gmres_ref.trace_array(p.trace[:k + 1]), _gmres_ref.trace_array(o.trace[:k + 1])
    assert not trace_close(tp, to, rtol=1e-10, atol=1e-13)


def test_indefinite_matrix_ends_in_invalid_preconditioner():
    ip, ix, d, rhs = system_of("indefinite", "float64")
    H = hierarchy_of("indefinite", "float64")
    assert [L.n for L in H.levels] == [480, 84]
    o = ref.cg(ip, ix, d, rhs, np.zeros(rhs.size), CG_MAX_ITER, 1e-10, prec=amg.Applier(H))
    assert (o.status, o.its) == (ref.INVALID_PRECOND, INDEFINITE[0]) and 0.5 < o.res / INDEFINITE[1] < 2


# ------------------------------------------------------------------------------------------------ 4. creation errors
def test_creation_errors():
    ip = np.array([0, 2, 4], np.int32); ix = np.array([0, 1, 0, 1], np.int32)
    assert amg.build(ip, ix, np.ones(4), ncols=3).status == amg.NOT_SQUARE
    for dt in ALL:
        H = amg.build(ip, ix, np.ones(4, dt))                # the coarse LU: u_11 = 1 - 1*1
        assert (H.status, H.row, H.levels) == (amg.ZERO_DIAGONAL, 1, None)
    # a missing diagonal and a zero diagonal report their (smallest) row
    ip3 = np.array([0, 2, 3, 5, 6], np.int32); ix3 = np.array([0, 1, 0, 1, 2, 2], np.int32)
    H = amg.build(ip3, ix3, np.ones(6))
    assert (H.status, H.row) == (amg.ZERO_DIAGONAL, 1)
    H = amg.build(ip, ix, np.array([1.0, 1.0, 1.0, 0.0]))
    assert (H.status, H.row) == (amg.ZERO_DIAGONAL, 1)
    H = amg.build(ip, ix, np.array([np.inf, 1.0, 1.0, 1.0]))
    assert (H.status, H.row) == (amg.ZERO_DIAGONAL, 0)
    # unsorted and duplicate columns, parameters out of range
    assert amg.build(ip, np.array([1, 0, 0, 1], np.int32), np.ones(4))[:2] == (amg.INVALID_ARGUMENT, 0)
    assert amg.build(ip, np.array([0, 1, 1, 1], np.int32), np.ones(4))[:2] == (amg.INVALID_ARGUMENT, 1)
    for kw in (dict(theta=-1.0), dict(coarse_max=0), dict(coarse_max=amg.COARSE_LIMIT + 1), dict(max_levels=0),
               dict(max_levels=amg.LEVELS_LIMIT + 1)):
        assert amg.build(ip, ix, np.array([2.0, 1.0, 1.0, 2.0]), **kw).status == amg.INVALID_ARGUMENT
