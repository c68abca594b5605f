"""The checker of mixed-precision refinement (tests/_refine_ref.py) checked on the CPU: it converges where the recurrence says it
must, in the counts measured with this very construction (numpy sums, tests/_cg_ref.py / tests/_gmres_ref.py as inner solvers in
f32 / c32) on gen.symmetric_banded(2000) and gen.hermitian_banded(1500, 3); its element-wise operations round as stated; its
events land where the recurrence says.  Nothing here touches the GPU: tests/test_gpu_refine.py holds the library to this checker."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_ref as cgref  # noqa: E402
import _refine_ref as ref  # noqa: E402

TOL = 1e-12


def _systems():
    from sprsolve_amd import gen
    return {"f64": gen.symmetric_banded(2000), "c64": gen.hermitian_banded(1500, 3)}


@pytest.fixture(scope="module")
def systems():
    return _systems()


def _diag(ip, ix, d):
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    return d[rows == ix].real.copy()


def _true_res(ip, ix, d, rhs, x):
    import scipy.sparse as sp
    n = rhs.size
    return np.linalg.norm(rhs - sp.csr_matrix((d, ix, ip), shape=(n, n)) @ x) / np.linalg.norm(rhs)


# measured with tests/_refine_ref.py (x0 = 0, tol 1e-12, max_outer 20, inner_max_iter 200): the inner CG counts per outer step
MEASURED = {("f64", 1e-4): [11, 12, 11], ("c64", 1e-4): [11, 11, 11],
            ("f64", 1e-2): [5, 6, 7, 6, 7, 6], ("c64", 1e-2): [5, 6, 6, 6, 6, 6]}


@pytest.mark.parametrize("inner_tol", [1e-4, 1e-2])
@pytest.mark.parametrize("name", ["f64", "c64"])
def test_counts_with_inner_cg(systems, name, inner_tol):
    ip, ix, d, rhs = systems[name]
    n = rhs.size
    o = ref.refine(ip, ix, d, rhs, np.zeros(n, d.dtype), 20, TOL, 200, inner_tol)
    print(name, inner_tol, o.outer, o.inner, o.hist)
    assert o.status == ref.OK
    assert o.outer == (3 if inner_tol == 1e-4 else 6)
    assert o.inner == MEASURED[(name, inner_tol)]
    assert o.res <= TOL and _true_res(ip, ix, d, rhs, o.x) <= TOL
    assert len(o.hist) == o.outer + 1 and all(b < a for a, b in zip(o.hist, o.hist[1:]))
    if (name, inner_tol) == ("f64", 1e-4):       # the residual history the feature was proposed with
        assert np.allclose(o.hist[1:], [5.6e-5, 2.4e-9, 1.8e-13], rtol=0.05)


@pytest.mark.parametrize("inner_tol", [1e-4, 1e-2])
@pytest.mark.parametrize("name", ["f64", "c64"])
def test_jacobi_gives_the_same_outer_counts(systems, name, inner_tol):
    ip, ix, d, rhs = systems[name]
    n = rhs.size
    o = ref.refine(ip, ix, d, rhs, np.zeros(n, d.dtype), 20, TOL, 200, inner_tol, precond_diag=_diag(ip, ix, d))
    assert o.status == ref.OK and o.outer == (3 if inner_tol == 1e-4 else 6)
    assert _true_res(ip, ix, d, rhs, o.x) <= TOL


@pytest.mark.parametrize("name", ["f64", "c64"])
def test_inner_gmres_converges_alike(systems, name):
    ip, ix, d, rhs = systems[name]
    n = rhs.size
    o = ref.refine(ip, ix, d, rhs, np.zeros(n, d.dtype), 20, TOL, 200, 1e-4, inner="gmres", restart=10)
    assert o.status == ref.OK and o.outer == 3 and _true_res(ip, ix, d, rhs, o.x) <= TOL


def test_f32_cg_alone_stalls_above_1e_8(systems):
    """What refinement is for: f32 CG reports convergence at 1e-12 (its recurrence residual), the true residual is 1.6e-7."""
    ip, ix, d, rhs = systems["f64"]
    n = rhs.size
    o = cgref.cg(ip, ix, d.astype(np.float32), rhs.astype(np.float32), np.zeros(n, np.float32), 200, 1e-12)
    true = _true_res(ip, ix, d, rhs, o.x.astype(np.float64))
    print("f32 CG: its %d reported %.2e true %.2e" % (o.its, o.res, true))
    assert o.status == cgref.OK and o.its == 31 and o.res <= 1e-12
    assert 1e-8 < true < 1e-6
    o64 = cgref.cg(ip, ix, d, rhs, np.zeros(n), 200, 1e-10)
    r = ref.refine(ip, ix, d, rhs, np.zeros(n), 20, TOL, 200, 1e-4)
    assert o64.its == 26 and sum(r.inner) < 3 * o64.its


def test_elementwise_roundings():
    rng = np.random.default_rng(5)
    v = rng.standard_normal(64) * 10.0 ** rng.integers(-20, 20, 64)
    got = ref.demote_scaled(v, 3.0, np.float32)
    assert got.dtype == np.float32 and np.array_equal(got, (v * 3.0).astype(np.float32))
    z = v[:32] + 1j * v[32:]
    gz = ref.demote_scaled(z, 0.5, np.complex64)
    assert np.array_equal(gz.real, (z.real * 0.5).astype(np.float32)) and np.array_equal(gz.imag, (z.imag * 0.5).astype(np.float32))
    # a real scale keeps the sign of a zero component, which a complex product by (scale + 0j) does not
    m = ref.demote_scaled(np.array([complex(-0.0, -1.0)]), 2.0, np.complex64)
    assert np.signbit(m.real[0]) and m.imag[0] == -2.0
    assert np.isposinf(ref.demote_scaled(np.array([1e300]), 1.0, np.float32)[0])
    assert np.isneginf(ref.demote_scaled(np.array([-1e30]), 1e30, np.float32)[0])
    e = rng.standard_normal(64).astype(np.float32)
    x = rng.standard_normal(64)
    assert np.array_equal(ref.axpy_promoted(x, e, 1e-7), x + e.astype(np.float64) * 1e-7)


def test_events(systems):
    ip, ix, d, rhs = systems["f64"]
    n = rhs.size
    z = np.zeros(n)
    o = ref.refine(ip, ix, d, np.zeros(n), np.full(n, 3.0), 20, TOL, 200, 1e-4)
    assert (o.status, o.outer, o.res) == (ref.OK, 0, 0.0) and not np.any(o.x)
    done = ref.refine(ip, ix, d, rhs, z, 20, TOL, 200, 1e-4)
    again = ref.refine(ip, ix, d, rhs, done.x, 20, TOL, 200, 1e-4)
    assert (again.status, again.outer, again.inner) == (ref.OK, 0, []) and np.array_equal(again.x, done.x)
    o = ref.refine(ip, ix, d, rhs, z, 1, TOL, 200, 1e-2, keep_iterates=True)
    assert (o.status, o.outer, o.inner) == (ref.INSUFFICIENT_ITER, 1, [5]) and np.array_equal(o.x, o.xs[0])
    assert 1e-3 < o.res < 1e-2
    # an inner solve that runs out of iterations still corrects
    o = ref.refine(ip, ix, d, rhs, z, 100, TOL, 2, 1e-4)
    assert (o.status, o.outer, sum(o.inner)) == (ref.OK, 24, 48) and _true_res(ip, ix, d, rhs, o.x) <= TOL
    # an indefinite matrix: inner CG breaks down in its first iteration, x is left alone
    neg = d.copy()
    rows = np.repeat(np.arange(n), np.diff(ip))
    neg[np.flatnonzero(rows == ix)[n // 2]] *= -1.0
    x0 = np.linspace(-1.0, 1.0, n)
    o = ref.refine(ip, ix, neg, rhs, x0, 20, TOL, 200, 1e-4)
    assert o.status == ref.BREAKDOWN and np.array_equal(o.x, x0), (o.status, o.outer, o.inner)
    assert ref.refine(ip, ix, d, rhs[:-1], z, 20, TOL, 200, 1e-4).status == ref.INCOMPATIBLE_RHS_SIZE
    assert ref.refine(ip, ix, d, rhs, np.zeros(n + 1), 20, TOL, 200, 1e-4).status == ref.INCOMPATIBLE_X_SIZE
    bad = rhs.copy(); bad[7] = np.nan
    assert ref.refine(ip, ix, d, bad, z, 20, TOL, 200, 1e-4).status == ref.BREAKDOWN
