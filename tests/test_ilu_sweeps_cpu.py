"""The Jacobi-sweep checker (tests/_ilu_sweeps_ref.py) checked on the CPU: with as many sweeps as the pattern has levels it
returns the exact folds of tests/_ilu_ref.py bit for bit, its k = 3 iteration counts (which tests/test_gpu_ilu_sweeps.py takes its
max_iter from) lie between the exact solve's and Jacobi's, and on a Hermitian positive-definite matrix its operator is Hermitian
positive definite up to rounding."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ilu_ref as ref  # noqa: E402
from _ilu_sweeps_ref import Sweeps, dense_operator  # noqa: E402
from test_ilu_cpu import ALL, C32, C64, CG_COUNTS, F32, F64, GMRES_COUNTS, GMRES_RESTART, bits, factors_of, tol_of  # noqa: E402

_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name

SWEEPS = 3
# the checker's counts with k = 3 sweeps, x0 = 0, f64 / c64 at tol 1e-10 and f32 / c32 at 1e-5 (CG_COUNTS' systems and rules)
SWEEP_CG_COUNTS = {"float64": 24, "complex128": 17, "float32": 9, "complex64": 10}
SWEEP_GMRES_COUNTS = {"float64": 48, "complex128": 48, "float32": 30, "complex64": 30}


# ------------------------------------------------------------------------------------------------ 1. the fixed point
FIXED_POINT_CASES = [("cd24x20", F64), ("cd24x20", F32), ("herm300", C64), ("herm300", C32), ("tri300", F64), ("ragged1000", F64),
                     ("cg", C64), ("indefinite", F64)]


@pytest.mark.parametrize("name,dt", FIXED_POINT_CASES, ids=_ids)
def test_as_many_sweeps_as_levels_is_the_exact_fold(name, dt):
    """A row of level l reads rows of lower levels only, and its fold is the exact solve's own expression: it holds its final
    bits from sweep l + 1 on."""
    ip, ix, d, rhs, f = factors_of(name, np.dtype(dt).name)
    exact = ref.Applier(ip, ix, f)
    for which, k in zip((1, 2), ref.level_counts(ip, ix)):
        got = Sweeps(ip, ix, f, k).solve(which, rhs)
        assert np.array_equal(bits(got), bits(exact.solve(which, rhs))), (which, k)


def test_fewer_sweeps_than_levels_is_another_operator():
    """(what makes the fixed point worth a test: k = 3 on 43 levels is not the exact solve)"""
    ip, ix, d, rhs, f = factors_of("cd24x20", "float64")
    exact = ref.Applier(ip, ix, f)
    for which in (0, 1, 2):
        assert not np.array_equal(Sweeps(ip, ix, f, SWEEPS).solve(which, rhs), exact.solve(which, rhs))
    one = Sweeps(ip, ix, f, 1)
    assert np.array_equal(bits(one.solve(1, rhs)), bits(rhs))                     # lower sweep 1 is the input
    dg = f[np.repeat(np.arange(rhs.size), np.diff(ip)) == ix]
    assert np.array_equal(bits(one.solve(2, rhs)), bits(rhs / dg)) and np.array_equal(bits(one.solve(0, rhs)), bits(rhs / dg))


# ------------------------------------------------------------------------------------------------ 2. iteration counts
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_sweeps_cg_count_lies_between_exact_and_jacobi(dt):
    ip, ix, d, rhs, f = factors_of("cg", np.dtype(dt).name)
    want = SWEEP_CG_COUNTS[np.dtype(dt).name]
    jacobi, exact = CG_COUNTS[np.dtype(dt).name]                                  # (recomputed by tests/test_ilu_cpu.py)
    o = ref.cg(ip, ix, d, rhs, np.zeros(rhs.size, dt), 2 * want, tol_of(dt), prec=Sweeps(ip, ix, f, SWEEPS))
    print("cg %s: Jacobi %d, %d sweeps %d, exact ILU(0) %d iterations" % (np.dtype(dt).name, jacobi, SWEEPS, o.its, exact))
    assert (o.status, o.its) == (ref.OK, want)
    assert exact <= o.its < jacobi


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_sweeps_gmres_count_lies_between_exact_and_jacobi(dt):
    ip, ix, d, rhs, f = factors_of("cd24x20", np.dtype(dt).name)
    want = SWEEP_GMRES_COUNTS[np.dtype(dt).name]
    jacobi, exact = GMRES_COUNTS[np.dtype(dt).name]
    o = ref.gmres(ip, ix, d, rhs, np.zeros(rhs.size, dt), 2 * want, tol_of(dt), restart=GMRES_RESTART, prec=Sweeps(ip, ix, f, SWEEPS))
    print("gmres %s: Jacobi %d, %d sweeps %d, exact ILU(0) %d steps" % (np.dtype(dt).name, jacobi, SWEEPS, o.its, exact))
    assert (o.status, o.its) == (ref.OK, want)
    assert exact <= o.its < jacobi


# ------------------------------------------------------------------------------------------------ 3. a Hermitian operator
def _asymmetry(M):
    return np.max(np.abs(M - M.conj().T)) / np.max(np.abs(M))


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_sweep_operator_is_hermitian_positive_definite_up_to_rounding(dt):
    """On a Hermitian positive-definite A, U = D L^H up to rounding, and the k-sweep operator is p(N)^H D^-1 p(N) with p the
    truncated Neumann series of the unit factor: Hermitian, and positive definite because p(N) is unit triangular.  The bound: ten
    times the exact operator's own relative asymmetry (the same quantity for folds of the same length; measured: at most five)."""
    ip, ix, d, rhs, f = factors_of("cg", np.dtype(dt).name)
    wide = np.complex128 if np.dtype(dt).kind == "c" else np.float64
    exact = ref.Applier(ip, ix, f)
    E = dense_operator(exact)
    col = rhs.size // 3
    assert np.array_equal(bits(E[:, col]), bits(exact.solve(0, np.eye(rhs.size, dtype=dt)[:, col])))   # the columns are the scalar path's
    base = _asymmetry(E.astype(wide))
    assert base > 0
    for k in (1, 2, 3, 4):
        M = dense_operator(Sweeps(ip, ix, f, k)).astype(wide)
        asym = _asymmetry(M)
        lam = np.linalg.eigvalsh((M + M.conj().T) / 2)[0]
        print("%s k = %d: asymmetry %.3e (exact %.3e, ratio %.2f), smallest eigenvalue %.4f" % (np.dtype(dt).name, k, asym, base, asym / base, lam))
        assert asym <= 10 * base
        assert lam > 0
