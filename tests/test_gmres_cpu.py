"""Restarted GMRES without a GPU: the C ABI and the Python mirror exist, and the numpy checker of the GPU tests
(tests/_gmres_ref.py) is checked independently of the library — its iterates minimise the residual over the Krylov space, its
residual estimate is the true residual, its events land where the header says — and the step counts the GPU tests quote
are recorded here."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gmres_ref as ref  # noqa: E402

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
NAMES = sorted(["sprs_gmres_%s_%s" % (f, s) for f in ("create", "solve", "precond_solve", "solve_dev") for s in "dzsc"] + ["sprs_gmres_destroy"])


@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_gmres_abi_and_binding_exist(L):
    src = open(os.path.join(ROOT, "include", "sprsolve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sprs_[a-z0-9_]+)\s*\(", src)) if n.startswith("sprs_gmres_"))
    assert declared == NAMES
    assert re.search(r"typedef\s+struct\s+sprs_gmres\s+sprs_gmres\s*;", src) and re.search(r"SPRS_SOLVER_GMRES\s*=\s*5\b", src)
    assert re.search(r"#define\s+SPRS_GMRES_MAX_RESTART\s+64\b", src)
    for name in NAMES:
        assert hasattr(L, name), name
    out = C.c_void_p()
    for s in "dzsc":
        want = L.sprs_bicgstab_create_d(None, 4, C.byref(out))               # what a null A answers today
        assert want == 7
        assert getattr(L, "sprs_gmres_create_" + s)(None, 4, 30, C.byref(out)) == want and not out.value
        assert getattr(L, "sprs_gmres_create_" + s)(None, 4, 65, C.byref(out)) == want and not out.value
        assert getattr(L, "sprs_gmres_solve_dev_" + s)(None, None, None, 4, None, 4, 10, 1e-8, None, None) == 7
    assert L.sprs_gmres_destroy(None) == 0
    assert L.sprs_solver_set_mode(None, 5, 1) == 7           # a null handle of the new kind
    import sprsolve_amd
    from sprsolve_amd import _lib
    assert sprsolve_amd.GMRES.NAME == "gmres" and sprsolve_amd.GMRES.KIND == _lib.SOLVER_GMRES == 5 and _lib.GMRES_MAX_RESTART == 64
    assert callable(sprsolve_amd.GMRES.solve) and callable(sprsolve_amd.GMRES.precond_solve)


def test_convection_diffusion_generator():
    from sprsolve_amd import gen
    ip, ix, d, rhs = gen.convection_diffusion_2d(6, 5, 0.3, 0.2)
    M = ref.dense(ip, ix, d)
    assert ip.dtype == ix.dtype == np.int32 and d.dtype == rhs.dtype == np.float64 and M.shape == (30, 30)
    assert np.all(np.diag(M) == 4.0) and not np.array_equal(M, M.T)
    r = 2 * 5 + 2                                            # interior point (i, j) = (2, 2)
    assert (M[r, r - 1], M[r, r + 1], M[r, r - 5], M[r, r + 5]) == (-1.3, -0.7, -1.2, -0.8) and np.count_nonzero(M[r]) == 5
    assert np.count_nonzero(M[0]) == 3
    i, j = np.divmod(np.arange(30), 5)
    assert np.allclose(M @ (1.0 + (i + 2.0 * j) / 11.0), rhs, rtol=1e-14)
    for dt in (C64, C32, F32):
        ipc, ixc, dc, rc = gen.convection_diffusion_2d(6, 5, 0.3, 0.2, dtype=dt)
        assert dc.dtype == rc.dtype == np.dtype(dt) and np.array_equal(ixc, ix)
        fac = (1 + 0.25j) if np.dtype(dt).kind == "c" else 1.0
        assert np.allclose(dc, d * fac, rtol=1e-6)


def _small_cases():
    from sprsolve_amd import gen
    for dt in (F64, C64):
        ip, ix, d, rhs = gen.convection_diffusion_2d(6, 5, dtype=dt)
        yield "cd6x5-" + np.dtype(dt).name, ip, ix, d, rhs
        ip, ix, d, rhs = gen.random_tridiagonal(12)
        if dt is C64:
            d = d * (1 + 0.25j); rhs = rhs * (1 - 0.5j)
        yield "tri12-" + np.dtype(dt).name, ip, ix, d.astype(dt), rhs.astype(dt)


@pytest.mark.parametrize("case", list(_small_cases()), ids=lambda c: c[0])
def test_iterates_minimise_the_residual_over_the_krylov_space(case):
    """Inside the first cycle the iterate after k steps is argmin |rhs - A x| over x0 + K_k(A, r0): numpy.linalg.lstsq on
    the explicitly built (orthonormalised) Krylov basis; and the estimate |g_k| is that residual's norm."""
    _, ip, ix, d, rhs = case
    n = rhs.size
    A = ref.dense(ip, ix, d)
    x0 = (0.1 * np.arange(n)).astype(d.dtype)
    steps = n - 2
    o = ref.gmres(ip, ix, d, rhs, x0, steps, 1e-30, restart=n, keep_iterates=True)
    assert o.status == ref.INSUFFICIENT_ITER and o.its == steps and len(o.xs) == steps
    assert np.array_equal(o.x, o.xs[-1])                     # max_iter reached: x holds the partial cycle's update
    r0 = rhs - A @ x0
    K = np.zeros((n, 0), d.dtype); v = r0
    for k in range(1, steps + 1):
        K = np.linalg.qr(np.concatenate([K, (v / np.linalg.norm(v))[:, None]], axis=1))[0]
        v = A @ K[:, -1]
        y = np.linalg.lstsq(A @ K, r0, rcond=None)[0]
        best = np.linalg.norm(r0 - A @ K @ y)
        got = np.linalg.norm(rhs - A @ o.xs[k - 1])
        assert got <= best * (1 + 1e-9) + 1e-13 * np.linalg.norm(rhs), (k, got, best)
        assert np.isclose(o.trace[k - 1][1], got, rtol=1e-8, atol=1e-13 * np.linalg.norm(rhs)), (k, o.trace[k - 1][1], got)
    gs = [t[1] for t in o.trace]
    assert all(b <= a * (1 + 1e-14) for a, b in zip(gs, gs[1:]))             # the residual never increases


def test_space_exhausted_exit():
    from sprsolve_amd import gen
    ip, ix, d, rhs = gen.random_tridiagonal(3)
    for dt in (F64, C64):
        o = ref.gmres(ip, ix, d.astype(dt), rhs.astype(dt), np.zeros(3, dt), 50, 1e-10, restart=5)
        assert o.status == ref.OK and 0 < o.its <= 3
        assert np.allclose(ref.dense(ip, ix, d) @ o.x, rhs, rtol=1e-12)
    # a diagonal matrix with two distinct eigenvalues: the Krylov space is exhausted after two steps with hn == 0 exactly
    ipd = np.arange(5, dtype=np.int32); ixd = np.arange(4, dtype=np.int32); dd = np.array([1.0, 1.0, 2.0, 2.0])
    o = ref.gmres(ipd, ixd, dd, np.ones(4), np.zeros(4), 50, 1e-14, restart=4)
    assert o.status == ref.OK and o.its <= 2 and np.allclose(o.x, 1.0 / dd, rtol=1e-14)
    ip1 = np.array([0, 1], np.int32); ix1 = np.array([0], np.int32)
    o = ref.gmres(ip1, ix1, np.array([4.0]), np.array([2.0]), np.zeros(1), 10, 1e-10, restart=5)
    assert (o.status, o.its) == (ref.OK, 1) and o.x[0] == 0.5 and o.trace[0][2] == 0.0       # hn == 0 at the first step


def test_checker_events():
    from sprsolve_amd import gen
    ip, ix, d, rhs = gen.convection_diffusion_2d(24, 20)
    n = rhs.size
    o = ref.gmres(ip, ix, d, np.zeros(n), np.ones(n), 100, 1e-10)
    assert (o.status, o.its, o.res) == (ref.OK, 0, 0.0) and not np.any(o.x)
    exact = np.linalg.solve(ref.dense(ip, ix, d), rhs)
    o = ref.gmres(ip, ix, d, rhs, exact, 100, 1e-10)
    assert (o.status, o.its) == (ref.OK, 0) and o.res <= 1e-10 and np.array_equal(o.x, exact)
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n), 2, 1e-10, restart=5)
    assert (o.status, o.its) == (ref.INSUFFICIENT_ITER, 2) and len(o.trace) == 2 and np.any(o.x)
    o10 = ref.gmres(ip, ix, d, rhs, np.zeros(n), 10, 1e-10, restart=5)       # max_iter hit exactly at a cycle end
    assert (o10.status, o10.its) == (ref.INSUFFICIENT_ITER, 10) and len(o10.trace) == 10
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n), 0, 1e-10)
    assert (o.status, o.its) == (ref.INSUFFICIENT_ITER, 0) and not np.any(o.x)
    assert ref.gmres(ip, ix, d, rhs[:-1], np.zeros(n), 10, 1e-10).status == ref.INCOMPATIBLE_RHS_SIZE
    assert ref.gmres(ip, ix, d, rhs, np.zeros(n + 1), 10, 1e-10).status == ref.INCOMPATIBLE_X_SIZE
    with pytest.raises(ValueError):
        ref.gmres(ip, ix, d, rhs, np.zeros(n), 10, 1e-10, restart=65)
    bad = rhs.copy(); bad[n // 3] = np.nan
    o = ref.gmres(ip, ix, d, bad, np.zeros(n), 8, 1e-10)
    assert (o.status, o.its) == (ref.BREAKDOWN, 0)


# ---- the cases of tests/test_gpu_gmres.py and the checker's step counts on them (x0 = 0; f64 / c64 at tol 1e-10, f32 / c32 at 1e-5)
def gpu_system(name, dt):
    from sprsolve_amd import gen
    cx = np.dtype(dt).kind == "c"
    if name == "tri1000":
        ip, ix, d, rhs = gen.random_tridiagonal(1000)
        if cx:
            d = d * (1 + 0.25j); rhs = rhs * (1 - 0.5j)
    else:
        r, c = {"cd24x20": (24, 20), "cd64x48": (64, 48)}[name]
        ip, ix, d, rhs = gen.convection_diffusion_2d(r, c, dtype=C64 if cx else F64)
    return ip, ix, d.astype(dt), rhs.astype(dt)


def is_single(dt):
    return np.dtype(dt) in (np.dtype(F32), np.dtype(C32))


def diag_of(ip, ix, d):
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    return d[rows == ix]


# (matrix, restart, Jacobi) -> steps for (f64, c64, f32, c32)
COUNTS = {
    ("cd24x20", 1, False): (577, 577, 310, 310), ("cd24x20", 5, False): (111, 111, 73, 73), ("cd24x20", 4, False): (133, 133, 77, 77),
    ("cd24x20", 8, False): (125, 125, 77, 77), ("cd24x20", 9, False): (119, 119, 70, 70), ("cd24x20", 30, False): (136, 136, 65, 65),
    ("cd24x20", 64, False): (99, 99, 52, 52),
    ("cd64x48", 5, False): (221, 221, 161, 161), ("cd64x48", 30, False): (328, 328, 199, 199),
    ("tri1000", 5, False): (20, 20, 10, 10), ("tri1000", 5, True): (19, 19, 9, 9),
    ("tri1000", 30, False): (20, 20, 10, 10), ("tri1000", 30, True): (18, 18, 9, 9),
}


# Trace rows compared at rtol 1e-9 / atol 1e-12 (by the self-check below and by the GPU tests, both modes): the first 40 of a
# solve, across its restarts — except on tri1000 with m = 5, whose residual falls by 1e-8 in 15 steps: the first 15 there.
# A restart forms rhs - A x with an absolute error of eps |rhs|, a relative one of eps |rhs| / |r|, which the following
# cycle's scalars inherit; measured with the checker against itself, sums taken pairwise, at a tenth of the tolerance
# (rtol 1e-10 / atol 1e-13): the first row outside is row 64 or later on the grids (of 99 .. 577), row 15 on tri1000 m = 5
# (of 19 .. 20), none on tri1000 m = 30.
TRACE_ROWS = {("tri1000", 5): 15}


def trace_rows(name, m):
    return TRACE_ROWS.get((name, m), 40)


def _self_check(name, m, dg, dt, want):
    """In f64 / c64 the checker with its sums taken pairwise stays inside the GPU tests' tolerances against itself: the same
    status, the same step count, res within rtol 1e-9 / atol 1e-12, x within 1e-7 max|x|, the trace rows of trace_rows()
    within rtol 1e-9 / atol 1e-12 — and within a tenth of that, which is how the prefix was chosen."""
    ip, ix, d, rhs = gpu_system(name, dt)
    n = rhs.size
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 2 * want, 1e-10, restart=m, precond_diag=dg)
    p = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 2 * want, 1e-10, restart=m, precond_diag=dg, sums="pairwise")
    assert p.status == o.status == ref.OK and p.its == o.its == want
    assert np.isclose(p.res, o.res, rtol=1e-9, atol=1e-12) and np.isclose(p.res, o.res, rtol=1e-10, atol=1e-13)
    assert np.max(np.abs(p.x - o.x)) <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
    k = min(trace_rows(name, m), o.its)
    assert k == o.its or k >= 15
    assert trace_close(ref.trace_array(p.trace[:k]), ref.trace_array(o.trace[:k]), rtol=1e-9, atol=1e-12)
    assert trace_close(ref.trace_array(p.trace[:k]), ref.trace_array(o.trace[:k]), rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("key", sorted(COUNTS), ids=lambda k: "%s-m%d-%s" % (k[0], k[1], "jacobi" if k[2] else "none"))
def test_step_counts_of_the_gpu_cases(key):
    """The counts the GPU file quotes; the checker's x meets the true-residual bound of the GPU tests (10 tol); and the
    self-check of the GPU tests' tolerances (_self_check)."""
    name, m, jac = key
    for dt, want in zip((F64, C64, F32, C32), COUNTS[key]):
        ip, ix, d, rhs = gpu_system(name, dt)
        n = rhs.size
        tol = 1e-5 if is_single(dt) else 1e-10
        dg = diag_of(ip, ix, d).real.astype(np.float32 if is_single(dt) else np.float64).copy() if jac else None
        o = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 4 * want, tol, restart=m, precond_diag=dg)
        assert (o.status, o.its) == (ref.OK, want), (np.dtype(dt).name, o.status, o.its)
        wide = np.complex128 if np.dtype(dt).kind == "c" else np.float64
        A = ref._matvec(ip, ix, d.astype(wide))
        assert np.linalg.norm(rhs.astype(wide) - A(o.x.astype(wide))) / np.linalg.norm(rhs.astype(wide)) <= 10 * tol
        if not is_single(dt):
            _self_check(name, m, dg, dt, want)


def test_self_check_with_a_complex_jacobi_diagonal():
    ip, ix, d, rhs = gpu_system("tri1000", C64)
    _self_check("tri1000", 5, diag_of(ip, ix, d), C64, 19)


def trace_close(a, b, rtol, atol):
    """Rows compared as [its, |g|, hn, R_jj, cs, s] with R_jj and s as the complex numbers they are."""
    def cx(t):
        t = np.atleast_2d(t)
        return np.concatenate([t[:, :3].astype(complex), (t[:, 3] + 1j * t[:, 4])[:, None], t[:, 5:6].astype(complex), (t[:, 6] + 1j * t[:, 7])[:, None]], axis=1)
    return a.shape == b.shape and np.allclose(cx(a), cx(b), rtol=rtol, atol=atol)
