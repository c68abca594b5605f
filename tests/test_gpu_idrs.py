"""IDR(s) on the GPU (sprs_idrs_*, csrc/idrs_fuse.hpp, idrs.hip) against the numpy restatement of its recurrence
(tests/_idrs_ref.py): the solver against the checker in all four scalar types, a harder convection-dominated grid, the loop
shapes of the kernels, tiny systems, the events, the applied preconditioners, the entry points and the argument checks.

Tolerances and margins are tests/test_gpu_gmres.py's: tol 1e-10 (f64 / c64) and 1e-5 (f32 / c32), a reported residual of at most
tol, a true residual (formed on the host in double) of at most 10 tol, trace rows at rtol 1e-9 / atol 1e-12 (1e-5 / 1e-8 in single
precision), step counts within max(5, its // 4) of the checker.  tests/test_idrs_cpu.py shows that the checker holds the step
and residual margins against itself under a change of summation order on every input used here.

The checker's product counts (x0 = 0): cd12x11 f64 s = 1, 4, 8: 62, 53, 52; f32: 38, 37, 33; csg9x8 c64: 48, 43, 41 (Jacobi 41,
36, 35); c32: 25, 24, 23 (Jacobi 23, 20, 20); cd24x22 (cx 2.0, cy 1.5) f64 s = 2, 4, 8: 92, 81, 75; c64: 86, 78, 74; cd31x29 s = 4:
108; cd96x90 s = 4: 246.

Every dot product and norm of the recurrence is accumulated in double from exact products, in the library and in the checker,
and the shadow space is orthonormalised in double in both: the scalars do not depend on the summation order beyond 1e-16, so
the first cycle's trace rows hold the single-precision tolerance too (with the sums in the scalar type the checker missed
it against itself by 5 to 66 times for s = 4 and 8)."""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_ref as cgref  # noqa: E402
import _idrs_ref as idr  # noqa: E402

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = idr.F64, idr.C64, idr.F32, idr.C32
ALL = [F64, C64, F32, C32]
_KNOBS = ("stream_nt",)
_id = lambda c: "%s-%s-s%d-%s" % (c[0], np.dtype(c[1]).name, c[2], "jacobi" if c[3] else "none")


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


@pytest.fixture(autouse=True)
def _restore_knobs(sa):
    ctx = sa.default_ctx(0)
    poll, grid = ctx.get("poll"), ctx.get("grid")
    yield
    for k in _KNOBS:
        ctx.set(k, -1)
    ctx.set("poll", poll); ctx.set("grid", grid)


def _single(dt):
    return np.dtype(dt) in (np.dtype(F32), np.dtype(C32))


def _true_res(ip, ix, d, rhs, x):
    wide = np.complex128 if np.dtype(rhs.dtype).kind == "c" else np.float64
    A = cgref._matvec(ip, ix, d.astype(wide))
    return float(np.linalg.norm(rhs.astype(wide) - A(x.astype(wide))) / np.linalg.norm(rhs.astype(wide)))


def _run(sa, solver, P, rhs, x, max_iter, tol):
    """-> (status, its, res) with the checker's status codes; x is updated in place."""
    E = sa.error
    try:
        its, res = solver.precond_solve(P, rhs, x, max_iter, tol) if P is not None else solver.solve(rhs, x, max_iter, tol)
        return idr.OK, its, res
    except E.InsufficientIterNum as e:
        return idr.INSUFFICIENT_ITER, e.iters, None
    except E.BreakDown as e:
        return idr.BREAKDOWN, e.its, None


def _jacobi(sa, diag, dt):
    if np.dtype(diag.dtype).kind == "c":
        return sa.DiagPrecond.new(np.ascontiguousarray(diag))             # complex V
    return sa.DiagPrecond.new(np.ascontiguousarray(diag), t_dtype=np.dtype(dt))


@functools.lru_cache(maxsize=None)
def _checker(name, dtname, s, pc, max_iter=2000):
    dt = np.dtype(dtname).type
    ip, ix, d, rhs, diag = idr.system(name, dt)
    o = idr.idrs((ip, ix, d), rhs, np.zeros(rhs.size, dt), max_iter, idr.tol_of(dt), s=s, precond_diag=diag if pc else None)
    o.x.setflags(write=False)
    return o


def _solve(sa, name, dt, s, pc, max_iter=2000, trace=0, x0=None):
    ip, ix, d, rhs, diag = idr.system(name, dt)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    solver = sa.IDRS.new(A, n, s)
    if trace:
        solver.set_trace(trace)
    P = _jacobi(sa, diag, dt) if pc else None
    x = np.zeros(n, dt) if x0 is None else x0.copy()
    st, its, res = _run(sa, solver, P, rhs, x, max_iter, idr.tol_of(dt))
    return st, its, res, x, solver.trace(), _true_res(ip, ix, d, rhs, x)


def _follows(sa, case):
    """Step count within the margin, both residual caps, one trace row per product, and the first cycle's s + 1 trace rows
    against the checker's at the trace tolerances."""
    name, dt, s, pc = case
    o = _checker(name, np.dtype(dt).name, s, pc)
    tol = idr.tol_of(dt)
    st, its, res, x, tr, true_res = _solve(sa, name, dt, s, pc, trace=400)
    want = idr.trace_array(o.trace)[:s + 1]
    rtol, atol = (1e-5, 1e-8) if _single(dt) else (1e-9, 1e-12)
    dev = np.max(np.abs(tr[:s + 1] - want) / (atol + rtol * np.abs(want))) if tr.shape[0] >= s + 1 else np.inf
    print("%s: its %d (checker %d, margin %d) res %.3e true %.3e (tol %g); first %d trace rows: worst |diff| / (atol + rtol |ref|) = %.3g"
          % (_id(case), its, o.its, idr.margin(o.its), res, true_res, tol, s + 1, dev))
    assert st == idr.OK and o.status == idr.OK
    assert abs(its - o.its) <= idr.margin(o.its)
    assert res <= tol and true_res <= 10 * tol
    assert tr.shape[0] == its and np.array_equal(tr[:, 0], np.arange(1, its + 1))
    assert np.array_equal(tr[:, 6] % (s + 1), np.arange(its) % (s + 1))     # k = 0 .. s - 1, then the omega step
    np.testing.assert_allclose(tr[:s + 1], want, rtol=rtol, atol=atol)


# ------------------------------------------------------------------------------------------------ 1. the checker, all four types
@pytest.mark.parametrize("case", idr.FOLLOW, ids=_id)
def test_follows_the_checker(sa, case):
    _follows(sa, case)


# ------------------------------------------------------------------------------------------------ 2. harder
@pytest.mark.parametrize("case", idr.HARDER, ids=_id)
def test_convection_dominated(sa, case):
    """cx = 2.0, cy = 1.5: the checks of 1, and fewer products with A than BiCGStab on the same operator (two an iteration)."""
    _follows(sa, case)
    name, dt, s, pc = case
    ip, ix, d, rhs, _ = idr.system(name, dt)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    x = np.zeros(n, dt)
    its = sa.IDRS.new(A, n, s).solve(rhs, x, 2000, 1e-10)[0]
    xb = np.zeros(n, dt)
    bits = sa.BiCGStab.new(A, n).solve(rhs, xb, 2000, 1e-10)[0]
    print("%s: IDR(%d) %d products, BiCGStab %d iterations = %d products" % (_id(case), s, its, bits, 2 * bits))
    assert its < 2 * bits


# ------------------------------------------------------------------------------------------------ 3. loop shapes
def test_several_packs_per_lane_and_the_chunked_walk(sa):
    """8640 rows on a grid of 8 workgroups: a lane walks several packs and each XCD its own chunk.  stream_nt 1 / 0 and poll 1 / 7
    give the same bits; its, res and x are those of the event."""
    case = ("cd96x90", F64, 4, False)
    ctx = sa.default_ctx(0)
    ctx.set("grid", 8)
    o = _checker("cd96x90", "float64", 4, False)
    runs = []
    for nt, poll in ((1, 1), (0, 1), (1, 7), (0, 7)):
        ctx.set("stream_nt", nt); ctx.set("poll", poll)
        runs.append(_solve(sa, *case))
    st, its, res, x, _, true_res = runs[0]
    print("cd96x90 grid 8: its %d (checker %d) res %.3e true %.3e" % (its, o.its, res, true_res))
    assert st == idr.OK and abs(its - o.its) <= idr.margin(o.its) and res <= 1e-10 and true_res <= 1e-9
    for r in runs[1:]:
        assert r[0] == st and r[1] == its and r[2] == res and r[3].tobytes() == x.tobytes()


def test_odd_rows(sa):
    """899 rows: a scalar tail behind the packs.  The same knobs, the same bits."""
    case = ("cd31x29", F64, 4, False)
    ctx = sa.default_ctx(0)
    o = _checker("cd31x29", "float64", 4, False)
    runs = []
    for nt, poll in ((1, 1), (0, 1), (1, 7)):
        ctx.set("stream_nt", nt); ctx.set("poll", poll)
        runs.append(_solve(sa, *case))
    st, its, res, x, _, true_res = runs[0]
    print("cd31x29: its %d (checker %d) res %.3e true %.3e" % (its, o.its, res, true_res))
    assert st == idr.OK and abs(its - o.its) <= idr.margin(o.its) and res <= 1e-10 and true_res <= 1e-9
    for r in runs[1:]:
        assert r[0] == st and r[1] == its and r[2] == res and r[3].tobytes() == x.tobytes()


# ------------------------------------------------------------------------------------------------ 4. tiny systems
def _dense_system(n, dt):
    rng = np.random.default_rng(100 + n)
    A = rng.standard_normal((n, n)) + 3.0 * np.eye(n)
    rhs = rng.standard_normal(n)
    if np.dtype(dt).kind == "c":
        A = A + 0.5j * rng.standard_normal((n, n)); rhs = rhs + 1j * rng.standard_normal(n)
    A = A.astype(dt); rhs = rhs.astype(dt)
    ip = np.arange(0, n * n + 1, n, dtype=np.int32)
    ix = np.tile(np.arange(n, dtype=np.int32), n)
    return A, ip, ix, np.ascontiguousarray(A.ravel()), rhs


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7])
def test_tiny_systems(sa, n, dt):
    """Finite termination: Ok within n + ceil(n / s) + 1 products, x the dense solve's (error at most cond(A) times the true-residual
    cap of 10 tol)."""
    A, ip, ix, d, rhs = _dense_system(n, dt)
    wide = np.complex128 if np.dtype(dt).kind == "c" else np.float64
    xs = np.linalg.solve(A.astype(wide), rhs.astype(wide))
    cond = np.linalg.cond(A.astype(wide))
    tol = idr.tol_of(dt)
    H = sa.HipCsr.new((n, n), ip, ix, d)
    for s in sorted({1, n}):
        bound = n + math.ceil(n / s) + 1
        x = np.zeros(n, dt)
        st, its, res = _run(sa, sa.IDRS.new(H, n, s), None, rhs, x, bound, tol)
        err = np.linalg.norm(x - xs) / np.linalg.norm(xs)
        print("n=%d s=%d %s: status %d its %s of %d res %s |x - x*| / |x*| %.3e (cond %.1f)" % (n, s, np.dtype(dt).name, st, its, bound, res, err, cond))
        assert st == idr.OK and its <= bound and res <= tol
        assert err <= 10 * tol * cond


# ------------------------------------------------------------------------------------------------ 5. events
def test_max_iter_mid_cycle(sa):
    """max_iter = 7 with s = 4: the second cycle's step k = 1.  x is the checker's, stopped at the same step."""
    o = _checker("cd12x11", "float64", 4, False, 7)
    st, its, res, x, tr, _ = _solve(sa, "cd12x11", F64, 4, False, max_iter=7, trace=16)
    assert o.status == idr.INSUFFICIENT_ITER and st == idr.INSUFFICIENT_ITER and its == 7 and tr.shape[0] == 7
    np.testing.assert_allclose(tr, idr.trace_array(o.trace), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(x, o.x, rtol=1e-9, atol=1e-12)
    # max_iter = 0: after the initial residual's test, x untouched
    x0 = np.full(132, 0.5)
    st, its, res, x, _, _ = _solve(sa, "cd12x11", F64, 4, False, max_iter=0, x0=x0)
    assert st == idr.INSUFFICIENT_ITER and its == 0 and np.array_equal(x, x0)


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_zero_rhs_and_converged_start(sa, dt):
    name = "csg9x8" if np.dtype(dt).kind == "c" else "cd12x11"
    ip, ix, d, rhs, _ = idr.system(name, dt)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    solver = sa.IDRS.new(A, n, 4)
    x = np.full(n, 3, dt)
    its, res = solver.solve(np.zeros(n, dt), x, 100, idr.tol_of(dt))
    assert its == 0 and res == 0 and not np.any(x)
    wide = np.complex128 if np.dtype(dt).kind == "c" else np.float64
    xs = np.linalg.solve(cgref.dense(ip, ix, d.astype(wide)), rhs.astype(wide)).astype(dt)
    x = xs.copy()
    loose = 1e-3 if _single(dt) else 1e-9                      # the rounded solution's residual: a few eps cond(A)
    its, res = solver.solve(rhs, x, 100, loose)
    assert its == 0 and res <= loose and np.array_equal(x, xs)


def test_singular_operator_breaks_down(sa):
    """A 2 x 2 system whose first row and column are zero: BreakDown, not a hang (every loop of the small solves is bounded by s)."""
    ip = np.array([0, 1, 2], np.int32); ix = np.array([0, 1], np.int32)
    for dt in ALL:
        d = np.array([0, 1], dt)
        A = sa.HipCsr.new((2, 2), ip, ix, d)
        for s in (1, 2):
            x = np.zeros(2, dt)
            st, its, res = _run(sa, sa.IDRS.new(A, 2, s), None, np.ones(2, dt), x, 50, idr.tol_of(dt))
            o = idr.idrs(cgref.dense(ip, ix, d), np.ones(2, dt), np.zeros(2, dt), 50, idr.tol_of(dt), s=s)
            print("singular %s s=%d: status %d its %d (checker %d, %d)" % (np.dtype(dt).name, s, st, its, o.status, o.its))
            assert st == idr.BREAKDOWN and o.status == idr.BREAKDOWN and 1 <= its <= 50 and np.all(np.isfinite(x))


# ------------------------------------------------------------------------------------------------ 6. applied preconditioners
@pytest.mark.parametrize("kind", ["ilu0_sweeps", "amg", "fsai"])
def test_applied_preconditioners(sa, kind):
    from sprsolve_amd import gen
    if kind == "fsai":
        ip, ix, d, rhs = gen.poisson3d(7, 6, 5)[:4]
    else:
        ip, ix, d, rhs, _ = idr.system("cd24x22m", F64)
    ip = ip.astype(np.int32); ix = ix.astype(np.int32); d = d.astype(F64); rhs = rhs.astype(F64)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    P = {"ilu0_sweeps": lambda: sa.ILU0.new(A, sweeps=3), "amg": lambda: sa.AMG.new(A), "fsai": lambda: sa.FSAI.new(A)}[kind]()
    solver = sa.IDRS.new(A, n, 4)
    x0 = np.zeros(n); xp = np.zeros(n)
    plain = solver.solve(rhs, x0, 2000, 1e-10)[0]
    its, res = solver.precond_solve(P, rhs, xp, 2000, 1e-10)
    true_res = _true_res(ip, ix, d, rhs, xp)
    dB, dX = sa.DevVec.from_numpy(rhs), sa.DevVec.from_numpy(np.zeros(n))
    dits, dres = solver.precond_solve(P, dB, dX, 2000, 1e-10)
    print("%s: %d products (%d without), res %.3e true %.3e" % (kind, its, plain, res, true_res))
    assert its < plain and res <= 1e-10 and true_res <= 1e-9
    assert (dits, dres) == (its, res) and dX.to_numpy().tobytes() == xp.tobytes()


def test_exact_ilu0(sa):
    ip, ix, d, rhs, _ = idr.system("cd24x22m", F64)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    solver = sa.IDRS.new(A, n, 4)
    x0 = np.zeros(n); xp = np.zeros(n)
    plain = solver.solve(rhs, x0, 2000, 1e-10)[0]
    its, res = solver.precond_solve(sa.ILU0.new(A), rhs, xp, 2000, 1e-10)
    assert its < plain and res <= 1e-10 and _true_res(ip, ix, d, rhs, xp) <= 1e-9


# ------------------------------------------------------------------------------------------------ 7. entry points and arguments
@pytest.mark.parametrize("dt", [F64, C32], ids=lambda d: np.dtype(d).name)
def test_device_and_host_entry_points_agree(sa, dt):
    name = "csg9x8" if np.dtype(dt).kind == "c" else "cd12x11"
    ip, ix, d, rhs, diag = idr.system(name, dt)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    solver = sa.IDRS.new(A, n, 4)
    tol = idr.tol_of(dt)
    for P in (None, _jacobi(sa, diag, dt)):
        x = np.zeros(n, dt)
        host = _run(sa, solver, P, rhs, x, 400, tol)
        x2 = np.zeros(n, dt)
        again = _run(sa, solver, P, rhs, x2, 400, tol)           # the workspace is reused: the same bits
        dB, dX = sa.DevVec.from_numpy(rhs), sa.DevVec.from_numpy(np.zeros(n, dt))
        dev = _run(sa, solver, P, dB, dX, 400, tol)
        assert host[0] == idr.OK and again == host and dev == host
        assert x2.tobytes() == x.tobytes() and dX.to_numpy().tobytes() == x.tobytes()


def test_arguments(sa):
    from sprsolve_amd import _lib
    from sprsolve_amd.error import IncompatibleMatrixFormat
    ip, ix, d, rhs, _ = idr.system("cd12x11", F64)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    assert sa.IDRS.new(A, n, 0).s_dim == 4
    x = np.zeros(n); x4 = np.zeros(n)
    a = sa.IDRS.new(A, n, 0).solve(rhs, x, 400, 1e-10)
    b = sa.IDRS.new(A, n, 4).solve(rhs, x4, 400, 1e-10)
    assert a == b and x.tobytes() == x4.tobytes()               # s = 0 is s = 4
    with pytest.raises(ValueError, match="SPRS_IDRS_MAX_S"):
        sa.IDRS.new(A, n, 9)
    with pytest.raises(ValueError):
        sa.IDRS.new(A, n, -1)
    ip2 = np.array([0, 1, 2], np.int32); ix2 = np.array([0, 1], np.int32)
    A2 = sa.HipCsr.new((2, 2), ip2, ix2, np.ones(2))
    with pytest.raises(ValueError, match="larger than the system"):
        sa.IDRS.new(A2, 2, 3)
    solver = sa.IDRS.new(A, n, 4)
    keep = np.full(n, 3.0)
    with pytest.raises(IncompatibleMatrixFormat, match="matrix size"):
        solver.solve(rhs[:-1], keep, 10, 1e-10)
    with pytest.raises(IncompatibleMatrixFormat, match="output vec"):
        solver.solve(rhs, np.full(n - 1, 3.0), 10, 1e-10)
    assert np.all(keep == 3.0)                                   # argument errors write nothing
    with pytest.raises(ValueError):
        solver.set_mode("literal")
    solver.set_mode("fused")
    assert _lib.lib().sprs_solver_set_mode(solver.h, _lib.SOLVER_IDRS, 1) == _lib.INVALID_ARGUMENT


def test_distributed_operator_is_refused(sa):
    import torch
    from sprsolve_amd import _lib, dist as sdist
    from test_gpu_dist import _self_halo_plan
    ctx = sa.default_ctx(0)
    dev = torch.device("cuda", 0)
    comm = sdist.Comm(ctx, 0, 1)
    try:
        ip, ix, d, rhs, _ = idr.system("cd12x11", F64)
        n = ip.size - 1
        plan = _self_halo_plan(torch, dev, n, ix, lambda c: np.zeros(c.shape, bool))
        A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip.copy()).to(dev), torch.from_numpy(d.copy()).to(dev), adopt=True,
                                    to_device=lambda a: torch.from_numpy(a).to(dev))
        h = C.c_void_p()
        st = _lib.lib().sprs_idrs_create_d(A.h, n, 4, C.byref(h))
        text = _lib.lib().sprs_last_error(ctx.h).decode()
        assert st == _lib.INVALID_ARGUMENT and not h.value and "distributed" in text, (st, text)
        with pytest.raises(ValueError, match="distributed"):
            sa.IDRS.new(A, n, 4)
    finally:
        comm.close()

