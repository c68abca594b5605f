"""The checker of the LSMR tests (tests/_lsmr_ref.py, the header's sprs_lsmr_* recurrence in numpy) checked itself: against
scipy.sparse.linalg.lsmr(atol = btol = tol, conlim = 0) — the same iteration count and x to rounding — and against
numpy.linalg.lstsq on the dense matrix.  No GPU.

Iteration counts of the checker at tol 1e-10 from x = 0 (ref.system(m, n, dtype, seed = m + n); consistent / inconsistent):
    f64   130x67 20 / 20   67x130 19 / 19   500x500 25 / 25   600x400 28 / 28
    c128  130x67 22 / 22   67x130 21 / 21   500x500 30 / 31   600x400 32 / 32
scipy took the same counts; |x - x_scipy| / |x| <= 3.3e-16; |x - x_lstsq| / |x_lstsq| <= 1.2e-9 (condition numbers 2.2 - 3.2)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lsmr_ref as ref  # noqa: E402

F64, C128 = np.float64, np.complex128
SHAPES = [(130, 67), (67, 130), (500, 500), (600, 400)]
MAX_ITER = 80                                                # >= 2 * 32, the largest count above
TOL = 1e-10


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _lstsq(D, b):
    return np.linalg.lstsq(D, b.astype(D.dtype), rcond=None)[0]


@pytest.mark.parametrize("consistent", [True, False], ids=["consistent", "inconsistent"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("dt", [F64, C128], ids=lambda d: np.dtype(d).name)
def test_checker_follows_scipy_and_lstsq(dt, shape, consistent):
    from scipy.sparse.linalg import lsmr as sp_lsmr
    m, n = shape
    ip, ix, d, b = ref.system(m, n, dt, seed=m + n, consistent=consistent)
    o = ref.lsmr(shape, ip, ix, d, b, np.zeros(n, dt), MAX_ITER, TOL)
    x_sp, istop, its_sp = sp_lsmr(ref.matrix(m, n, ip, ix, d), b, atol=TOL, btol=TOL, conlim=0, maxiter=MAX_ITER)[:3]
    xl = _lstsq(ref.dense(m, n, ip, ix, d), b)               # over-determined: least squares; under-determined: minimum norm
    print("%s %dx%d: its %d (scipy %d, istop %d) |x - scipy| %.2e |x - lstsq| %.2e" % (np.dtype(dt).name, m, n, o.its, its_sp, istop,
                                                                                   _rel(o.x, x_sp), _rel(o.x, xl)))
    assert o.status == ref.OK and istop in (1, 2)
    assert o.its == its_sp and 2 * o.its <= MAX_ITER
    assert _rel(o.x, x_sp) <= 1e-13                          # the same recurrence: rounding only (measured <= 3.3e-16)
    assert _rel(o.x, xl) <= 1e-8                             # tol 1e-10 times the condition number, with room (measured <= 1.2e-9)
    # what the recurrence reports against the true residuals
    D = ref.dense(m, n, ip, ix, d)
    r = b - D @ o.x
    assert np.isclose(o.res, np.linalg.norm(r) / np.linalg.norm(b), rtol=1e-6, atol=1e-12)
    truly_inconsistent = not consistent and m > n            # a square or under-determined full-rank system has a solution anyway
    assert (o.res <= 10 * TOL) != truly_inconsistent
    if truly_inconsistent:
        assert o.ares <= TOL


@pytest.mark.parametrize("dt", [F64, C128], ids=lambda d: np.dtype(d).name)
def test_damped_against_lstsq_on_the_stacked_matrix(dt):
    m, n, lam = 130, 67, 0.7
    ip, ix, d, b = ref.system(m, n, dt, seed=5, consistent=False)
    o = ref.lsmr((m, n), ip, ix, d, b, np.zeros(n, dt), MAX_ITER, TOL, damp=lam)
    D = ref.dense(m, n, ip, ix, d)
    xl = _lstsq(np.vstack([D, lam * np.eye(n)]), np.concatenate([b, np.zeros(n, dt)]))
    print("damped %s: its %d |x - lstsq| %.2e" % (np.dtype(dt).name, o.its, _rel(o.x, xl)))
    assert o.status == ref.OK and 2 * o.its <= MAX_ITER
    assert _rel(o.x, xl) <= 1e-8


@pytest.mark.parametrize("dt", [F64, C128], ids=lambda d: np.dtype(d).name)
def test_initial_guess(dt):
    m, n = 130, 67
    ip, ix, d, b = ref.system(m, n, dt, seed=6, consistent=False)
    xl = _lstsq(ref.dense(m, n, ip, ix, d), b)
    cold = ref.lsmr((m, n), ip, ix, d, b, np.zeros(n, dt), MAX_ITER, TOL)
    x0 = (xl * (1 + 1e-4)).astype(dt)
    warm = ref.lsmr((m, n), ip, ix, d, b, x0, MAX_ITER, TOL)
    print("initial guess %s: its %d (from zero %d) |x - lstsq| %.2e" % (np.dtype(dt).name, warm.its, cold.its, _rel(warm.x, xl)))
    assert warm.status == ref.OK and warm.its < cold.its
    assert _rel(warm.x, xl) <= 1e-8
    exact = ref.lsmr((m, n), ip, ix, d, (ref.dense(m, n, ip, ix, d) @ xl).astype(dt), xl.astype(dt), MAX_ITER, TOL)
    assert exact.status == ref.OK and exact.its <= 1          # nothing (or rounding noise) is left to correct


@pytest.mark.parametrize("dt", [F64, C128], ids=lambda d: np.dtype(d).name)
def test_lucky_termination(dt):
    n = 8
    ip = np.arange(n + 1, dtype=np.int32); ix = np.arange(n, dtype=np.int32)
    d = (np.arange(n) + 2.0).astype(dt)
    b = np.zeros(n, dt); b[3] = 1.0
    o = ref.lsmr((n, n), ip, ix, d, b, np.zeros(n, dt), 10, TOL)
    assert (o.status, o.its) == (ref.OK, 1)                  # beta = 0 in the first iteration: the exact solution
    want = np.zeros(n, dt); want[3] = 1.0 / d[3]
    assert np.allclose(o.x, want, rtol=1e-15, atol=0)


def test_events_and_argument_checks():
    m, n = 130, 67
    ip, ix, d, b = ref.system(m, n, F64, seed=7)
    z = np.zeros(n)
    assert ref.lsmr((m, n), ip, ix, d, b, z, 3, TOL)[:2] == (ref.INSUFFICIENT_ITER, 3)
    o = ref.lsmr((m, n), ip, ix, d, np.zeros(m), np.ones(n), 10, TOL)
    assert (o.status, o.its) == (ref.OK, 0) and not o.x.any()                  # zero rhs: x = 0
    bad = b.copy(); bad[5] = np.nan
    assert ref.lsmr((m, n), ip, ix, d, bad, z, 10, TOL).status == ref.BREAKDOWN
    assert ref.lsmr((m, n), ip, ix, d, b[:-1], z, 10, TOL).status == ref.DIM_MISMATCH
    assert ref.lsmr((m, n), ip, ix, d, b, np.zeros(n + 1), 10, TOL).status == ref.DIM_MISMATCH
    assert ref.lsmr((m, n), ip, ix, d, b, z, 10, TOL, damp=-1.0).status == ref.INVALID_ARGUMENT
