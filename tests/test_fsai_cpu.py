"""The FSAI checker (tests/_fsai_ref.py) checked on the CPU against independent arithmetic: every row against np.linalg.solve,
diag(G A G^H) = 1, G^H G = A^-1 where the pattern is the whole lower triangle, its creation errors, and the iteration counts of
the project's checkers (tests/_ilu_ref.py's cg — tests/_cg_ref.py's with the preconditioner as a callable — and gmres,
tests/_krylov_prec_ref.py's bicgstab and minres) under its apply.  Those counts stand behind every max_iter of
tests/test_gpu_fsai.py: at least twice the count, the rule of tests/test_gpu_cg.py.  The systems, the checker's factors and runs
and the trace prefixes of the GPU file are built here, once, and shared read-only."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fsai_ref as fr  # noqa: E402
import _ilu_ref as ref  # noqa: E402
import _krylov_prec_ref as kp  # noqa: E402
from test_ilu_cpu import ALL, C32, C64, F32, F64, CG_COUNTS, bits, cg_system, indefinite_system, is_single, tol_of  # noqa: E402,F401
from test_krylov_prec_cpu import gpu_tols, rows_close  # noqa: E402

_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name
SYSTEMS = ("cg", "banded")
POWERS = (1, 2)
GMRES_RESTART = 10

# the checkers' counts, x0 = 0, f64 / c64 at tol 1e-10 and f32 / c32 at 1e-5.  CG: (Jacobi, FSAI power 1, FSAI power 2)
FSAI_CG_COUNTS = {
    "cg": {"float64": (44, 31, 23), "complex128": (41, 22, 16), "float32": (23, 12, 9), "complex64": (23, 12, 9)},
    "banded": {"float64": (22, 10, 6), "complex128": (21, 10, 6), "float32": (11, 5, 3), "complex64": (11, 5, 3)},
}
# power 1: BiCGStab, MINRES, GMRES(10)
FSAI_KRYLOV_COUNTS = {
    "cg": {"float64": (22, 30, 39), "complex128": (15, 21, 27), "float32": (9, 11, 12), "complex64": (8, 11, 13)},
    "banded": {"float64": (6, 9, 10), "complex128": (6, 9, 9), "float32": (3, 4, 5), "complex64": (3, 4, 5)},
}
_SOLVER_COL = {"bicgstab": 0, "minres": 1, "gmres": 2}


def eps_of(dt):
    return float(np.finfo(np.float32 if is_single(dt) else np.float64).eps)


# ------------------------------------------------------------------------------------------------ the systems
@functools.lru_cache(maxsize=None)
def system(name, dtname):
    """"cg": tests/test_ilu_cpu.py's cg_system; "banded": symmetric_banded(300) for the real types, hermitian_banded(300) for the
    complex ones; "p3_64x64x8": poisson3d(64, 64, 8), 32 768 rows of 1 .. 4 entries in G; "indefinite"."""
    from sprsolve_amd import gen
    dt = np.dtype(dtname).type
    if name == "cg":
        ip, ix, d, rhs = cg_system(dt)
    elif name == "banded":
        ip, ix, d, rhs = (gen.hermitian_banded if np.dtype(dt).kind == "c" else gen.symmetric_banded)(300)
    elif name == "p3_64x64x8":
        ip, ix, d, rhs = gen.poisson3d(64, 64, 8)
    elif name == "indefinite":
        ip, ix, d, rhs = indefinite_system()
    else:
        raise KeyError(name)
    ip = ip.astype(np.int32); ix = ix.astype(np.int32); d = d.astype(dt); rhs = rhs.astype(dt)
    for a in (ip, ix, d, rhs):
        a.setflags(write=False)
    return ip, ix, d, rhs


@functools.lru_cache(maxsize=None)
def dense_hpd(n, dtname):
    """A dense Hermitian positive-definite n x n matrix stored as full CSR: B B^H / n + I, B seeded uniform."""
    from sprsolve_amd import gen
    dt = np.dtype(dtname)
    B = gen.uniform(gen.SEED, n * n, stream=90).reshape(n, n)
    if dt.kind == "c":
        B = B + 1j * gen.uniform(gen.SEED, n * n, stream=91).reshape(n, n)
    A = B @ B.conj().T / n + np.eye(n)
    A = ((A + A.conj().T) / 2).astype(dt)
    A[np.arange(n), np.arange(n)] = A.diagonal().real
    ip = (np.arange(n + 1) * n).astype(np.int32); ix = np.tile(np.arange(n, dtype=np.int32), n); d = A.reshape(-1).copy()
    rhs = gen.uniform(gen.SEED, n, stream=92).astype(dt)
    for a in (ip, ix, d, rhs):
        a.setflags(write=False)
    return ip, ix, d, rhs


@functools.lru_cache(maxsize=None)
def factor_of(name, dtname, power):
    """The checker's G of a named system (or of "dense<n>"), computed once and shared (read-only)."""
    ip, ix, d, _ = dense_hpd(int(name[5:]), dtname) if name.startswith("dense") else system(name, dtname)
    f = fr.fsai(ip, ix, d, power)
    assert f.status == fr.OK, (name, dtname, power, f[:2])
    for a in (f.ip, f.ix, f.val):
        a.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def applier(name, dtname, power):
    f = factor_of(name, dtname, power)
    return fr.Applier(f.ip, f.ix, f.val)


def max_iter_of(solver, name, dtname, power=1):
    """At least twice the checker's count (tests/test_gpu_cg.py's rule)."""
    if solver == "cg":
        return 2 * FSAI_CG_COUNTS[name][dtname][power]
    assert power == 1
    return 2 * FSAI_KRYLOV_COUNTS[name][dtname][_SOLVER_COL[solver]] + 2


@functools.lru_cache(maxsize=None)
def checker_run(solver, name, dtname, power=1, sums="numpy"):
    ip, ix, d, rhs = system(name, dtname)
    dt = np.dtype(dtname).type
    x0 = np.zeros(rhs.size, dt)
    mi, tol, M = max_iter_of(solver, name, dtname, power), tol_of(dt), applier(name, dtname, power)
    if solver == "cg":
        assert sums == "numpy"
        return ref.cg(ip, ix, d, rhs, x0, mi, tol, prec=M)
    if solver == "gmres":
        return ref.gmres(ip, ix, d, rhs, x0, mi, tol, restart=GMRES_RESTART, prec=M, sums=sums)
    o = getattr(kp, solver)(ip, ix, d, rhs, x0, mi, tol, prec=M, sums=sums)
    o.x.setflags(write=False); o.trace.setflags(write=False)
    return o


def gmres_trace_array(trace):
    return np.array([[t[0], t[1], t[2], t[3].real, t[3].imag, t[4], t[5].real, t[5].imag] for t in trace]).reshape(-1, 8)


@functools.lru_cache(maxsize=None)
def trace_prefix(solver, name, dtname):
    """The trace rows the GPU test may compare (tests/test_krylov_prec_cpu.py::trace_prefix, the rule of tests/test_ilu_cpu.py's
    GMRES_TRACE_ROWS): the leading rows on which the checker against itself with its sums taken pairwise holds a TENTH of the GPU
    tolerance."""
    rtol, atol = gpu_tols(np.dtype(dtname).type)
    a, b = checker_run(solver, name, dtname), checker_run(solver, name, dtname, 1, "pairwise")
    if solver == "gmres":
        from test_gmres_cpu import trace_close
        ta, tb = gmres_trace_array(a.trace), gmres_trace_array(b.trace)
        k = 0
        while k < min(len(ta), len(tb)) and trace_close(ta[:k + 1], tb[:k + 1], rtol=rtol / 10, atol=atol / 10):
            k += 1
        return k
    return rows_close(a.trace, b.trace, rtol / 10, atol / 10)


# ------------------------------------------------------------------------------------------------ 1. independent arithmetic
def _wide(a):
    return a.astype(np.complex128 if a.dtype.kind == "c" else np.float64)


@pytest.mark.parametrize("power", POWERS)
@pytest.mark.parametrize("dt", ALL, ids=_ids)
@pytest.mark.parametrize("name", SYSTEMS)
def test_rows_against_linalg_solve_and_unit_diagonal(name, dt, power):
    """Row i is conj(y) / sqrt(y_last) with S y = e_last, S = A(J_i, J_i) (the last column of C^-H is y / sqrt(y_last)):
    relative error at most 64 eps; and diag(G A G^H) = 1 within 64 eps."""
    dtname = np.dtype(dt).name
    ip, ix, d, _ = system(name, dtname)
    f = factor_of(name, dtname, power)
    n = ip.size - 1
    A = _wide(fr.dense(ip, ix, d))
    A = np.tril(A) + np.tril(A, -1).conj().T                 # only the lower triangle is ever read
    worst = 0.0
    for i in range(n):
        J = f.ix[f.ip[i]:f.ip[i + 1]]
        e = np.zeros(J.size); e[-1] = 1.0
        y = np.linalg.solve(A[np.ix_(J, J)], e)
        want = np.conj(y) / np.sqrt(y[-1].real)
        worst = max(worst, np.max(np.abs(_wide(f.val[f.ip[i]:f.ip[i + 1]]) - want)) / np.max(np.abs(want)))
    G = _wide(fr.dense(f.ip, f.ix, f.val))
    dg = np.max(np.abs(np.diag(G @ A @ G.conj().T) - 1))
    print("fsai %s %s power %d: rows %.2e, |diag - 1| %.2e, longest row %d" % (name, dtname, power, worst, dg, np.diff(f.ip).max()))
    assert worst <= 64 * eps_of(dt) and dg <= 64 * eps_of(dt)
    assert np.all(f.ix[f.ip[1:] - 1] == np.arange(n)) and np.all(f.val[f.ip[1:] - 1].imag == 0) and np.all(f.val[f.ip[1:] - 1].real > 0)


def test_pattern_of_power_two_is_the_structural_square():
    import scipy.sparse as sp
    ip, ix, d, _ = system("banded", "float64")
    n = ip.size - 1
    P = sp.csr_matrix((np.ones(d.size), ix, ip), shape=(n, n))
    P2 = sp.tril(P @ P).tocsr(); P2.sort_indices()
    f = factor_of("banded", "float64", 2)
    assert np.array_equal(f.ip, P2.indptr) and np.array_equal(f.ix, P2.indices)
    f1 = factor_of("banded", "float64", 1)
    P1 = sp.tril(P).tocsr(); P1.sort_indices()
    assert np.array_equal(f1.ip, P1.indptr) and np.array_equal(f1.ix, P1.indices)


@pytest.mark.parametrize("dt", [F64, C64], ids=_ids)
def test_dense_pattern_gives_the_inverse(dt):
    """Where J_i is the whole lower triangle, G^H G = A^-1: |G^H G A - I|_max <= 1e-13 on a dense 24 x 24 matrix."""
    dtname = np.dtype(dt).name
    ip, ix, d, rhs = dense_hpd(24, dtname)
    f = factor_of("dense24", dtname, 1)
    assert np.array_equal(np.diff(f.ip), np.arange(1, 25))
    A = fr.dense(ip, ix, d); G = fr.dense(f.ip, f.ix, f.val)
    err = np.max(np.abs(G.conj().T @ G @ A - np.eye(24)))
    print("dense24 %s: cond %.1f, |G^H G A - I| %.2e" % (dtname, np.linalg.cond(A), err))
    assert err <= 1e-13
    # ... and the apply is that product, folded
    M = applier("dense24", dtname, 1)
    v = A @ rhs
    assert np.max(np.abs(M(v) - rhs)) <= 1e-12 * np.max(np.abs(rhs))


@pytest.mark.parametrize("dt", [F64, C32], ids=_ids)
def test_adjoint_and_apply(dt):
    """GH is G's conjugate transpose with each row's entries in ascending column, and the apply is GH (G v) to rounding."""
    import scipy.sparse as sp
    dtname = np.dtype(dt).name
    f = factor_of("cg", dtname, 2)
    n = f.ip.size - 1
    hp, hx, hv = fr.adjoint(f.ip, f.ix, f.val)
    want = sp.csr_matrix((f.val, f.ix, f.ip), shape=(n, n)).conj().T.tocsr(); want.sort_indices()
    assert np.array_equal(hp, want.indptr) and np.array_equal(hx, want.indices) and np.array_equal(bits(hv), bits(want.data))
    _, _, _, rhs = system("cg", dtname)
    G = _wide(fr.dense(f.ip, f.ix, f.val))
    out = applier("cg", dtname, 2)(rhs)
    assert out.dtype == np.dtype(dt)
    assert np.max(np.abs(_wide(out) - G.conj().T @ (G @ _wide(rhs)))) <= 64 * eps_of(dt) * np.max(np.abs(out))


# ------------------------------------------------------------------------------------------------ 2. creation errors
def test_indefinite_matrix_is_not_positive_definite_on_the_pattern():
    ip, ix, d, _ = system("indefinite", "float64")
    for power in POWERS:
        f = fr.fsai(ip, ix, d, power)
        assert (f.status, f.row, f.val) == (fr.INVALID_PRECOND, 15, None)
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    assert d[(rows == ix) & (rows == 15)][0] == -4.0 and np.all(d[(rows == ix) & (rows < 15)] > 0)


def test_missing_diagonal_reports_its_row():
    ip, ix, d, _ = system("banded", "float64")
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    for row in (0, 137, 299):
        keep = ~((rows == row) & (ix == row))
        ip2 = np.zeros_like(ip); np.cumsum(np.bincount(rows[keep], minlength=ip.size - 1), out=ip2[1:])
        for power in POWERS:                                  # (with power 2 row 137 is still in its own pattern: a(137, 137) is what is missing)
            f = fr.fsai(ip2, ix[keep], d[keep], power)
            assert (f.status, f.row) == (fr.ZERO_DIAGONAL, row)
    # a zero diagonal wins over a row that is not positive definite
    ipi, ixi, di, _ = system("indefinite", "float64")
    ri = np.repeat(np.arange(ipi.size - 1), np.diff(ipi))
    keep = ~((ri == 40) & (ixi == 40))
    ip2 = np.zeros_like(ipi); np.cumsum(np.bincount(ri[keep], minlength=ipi.size - 1), out=ip2[1:])
    assert fr.fsai(ip2, ixi[keep], di[keep], 1)[:2] == (fr.ZERO_DIAGONAL, 40)


def test_row_cap_and_unsorted_columns():
    ip, ix, d, _ = dense_hpd(70, "float64")
    f = fr.fsai(ip, ix, d, 1)
    assert (f.status, f.row) == (fr.INVALID_ARGUMENT, 64)    # row 64 is the first with 65 entries
    ipb = np.array([0, 2, 4], np.int32)
    assert fr.fsai(ipb, np.array([1, 0, 0, 1], np.int32), np.ones(4))[:2] == (fr.INVALID_ARGUMENT, 0)
    assert fr.fsai(ipb, np.array([0, 1, 1, 1], np.int32), np.ones(4))[:2] == (fr.INVALID_ARGUMENT, 1)
    # a non-finite or non-positive d
    assert fr.fsai(ipb, np.array([0, 1, 0, 1], np.int32), np.array([1.0, 1.0, 1.0, 1.0]))[:2] == (fr.INVALID_PRECOND, 1)   # 1 - 1*1
    assert fr.fsai(ipb, np.array([0, 1, 0, 1], np.int32), np.array([np.inf, 1.0, 1.0, 4.0]))[:2] == (fr.INVALID_PRECOND, 0)


def test_long_band_squared_stays_under_the_cap():
    from sprsolve_amd import gen
    ip, ix, d, _ = gen.symmetric_banded(2000, hbw=8)
    J = fr.pattern(ip, ix, 2)
    assert max(j.size for j in J) == 17


# ------------------------------------------------------------------------------------------------ 3. iteration counts
@pytest.mark.parametrize("dt", ALL, ids=_ids)
@pytest.mark.parametrize("name", SYSTEMS)
def test_cg_counts(name, dt):
    dtname = np.dtype(dt).name
    ip, ix, d, rhs = system(name, dtname)
    want_j, want_1, want_2 = FSAI_CG_COUNTS[name][dtname]
    oj = ref.cg(ip, ix, d, rhs, np.zeros(rhs.size, dt), 2 * want_j, tol_of(dt), prec=ref.jacobi(ip, ix, d))
    o1, o2 = checker_run("cg", name, dtname, 1), checker_run("cg", name, dtname, 2)
    print("cg %s %s: Jacobi %d, FSAI(1) %d, FSAI(2) %d iterations" % (name, dtname, oj.its, o1.its, o2.its))
    assert [(o.status, o.its) for o in (oj, o1, o2)] == [(ref.OK, want_j), (ref.OK, want_1), (ref.OK, want_2)]
    assert o1.its < oj.its and o2.its <= o1.its
    if name == "cg":
        assert want_j == CG_COUNTS[dtname][0]                # the Jacobi column of tests/test_ilu_cpu.py


@pytest.mark.parametrize("dt", ALL, ids=_ids)
@pytest.mark.parametrize("name", SYSTEMS)
def test_bicgstab_minres_gmres_counts(name, dt):
    dtname = np.dtype(dt).name
    got = tuple(checker_run(s, name, dtname) for s in ("bicgstab", "minres", "gmres"))
    print("fsai(1) %s %s: BiCGStab %d, MINRES %d, GMRES(10) %d" % ((name, dtname) + tuple(o.its for o in got)))
    assert all(o.status == ref.OK for o in got)
    assert tuple(o.its for o in got) == FSAI_KRYLOV_COUNTS[name][dtname]


@pytest.mark.parametrize("solver", ["bicgstab", "minres", "gmres"])
def test_trace_prefix_of_the_gpu_cases(solver):
    """Every GPU case keeps at least one comparable row, the f64 ones at least five (tests/test_gpu_krylov_prec.py's floor)."""
    for name in SYSTEMS:
        for dt in ALL:
            k = trace_prefix(solver, name, np.dtype(dt).name)
            print("prefix %s %s %s: %d of %d" % (solver, name, np.dtype(dt).name, k, len(checker_run(solver, name, np.dtype(dt).name).trace)))
            assert k >= (5 if np.dtype(dt) == np.dtype(F64) and name == "cg" else 1)
