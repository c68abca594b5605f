"""Batched conjugate gradients (sprs_cgmany_*, csrc/cg_many_fuse.hpp) against the per-column checker (tests/_cg_many_ref.py):
every dtype with and without Jacobi, the independence of the columns, the events of the recurrence in one solve, the entry points.

The checker's iteration counts (x0 = 0; f64 / c64 at tol 1e-10, f32 / c32 at 1e-5) on the columns used here — the generator's
rhs, gen.uniform(SEED + s, n) for s = 1..7 and the unit vector e_{n/2}:
    f64 26 (Jacobi 22-23), unit vector 20 (19);   f32 13-14 (11-12), unit vector 11 (9);
    c64 25-26 (23-24), unit vector 22 (22);       c32 12-13 (11-12).
MAX_ITER = 80 is at least three times the largest."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_many_ref as many  # noqa: E402
import _cg_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
MAX_ITER = 80                                                # >= 3 * 26, the largest count above


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


@pytest.fixture(autouse=True)
def _restore_poll(sa):
    ctx = sa.default_ctx(0)
    poll = ctx.get("poll")
    yield
    ctx.set("poll", poll)


def _is_single(dt):
    return np.dtype(dt) in (np.dtype(F32), np.dtype(C32))


def _tol(dt):
    return 1e-5 if _is_single(dt) else 1e-10


_sys_cache, _ref_cache = {}, {}


def _system(dt):
    """-> (ip, ix, d, B): test_gpu_cg.py's systems and the nine columns [rhs, uniform 1..7, e_{n/2}] in the dtype under test."""
    key = np.dtype(dt).name
    if key not in _sys_cache:
        from sprsolve_amd import gen
        cx = np.dtype(dt).kind == "c"
        ip, ix, d, rhs = gen.hermitian_banded(1500, 3) if cx else gen.symmetric_banded(2000)
        n = rhs.size
        cols = [rhs]
        for s in range(1, 8):
            u = gen.uniform(gen.SEED + s, n)
            cols.append(u + 1j * gen.uniform(gen.SEED + s, n, stream=1) if cx else u)
        cols.append(np.eye(1, n, n // 2)[0])
        _sys_cache[key] = (ip, ix, d.astype(dt), np.stack(cols, axis=1).astype(dt))
    return _sys_cache[key]


def _diag(ip, ix, d):
    dg = d[np.repeat(np.arange(ip.size - 1), np.diff(ip)) == ix]
    return dg.real.astype(F32 if _is_single(d.dtype) else F64).copy()


def _checker(dt, pc):
    """The checker on all nine columns, once per (dtype, preconditioner)."""
    key = (np.dtype(dt).name, pc)
    if key not in _ref_cache:
        ip, ix, d, B = _system(dt)
        _ref_cache[key] = many.cg_many(ip, ix, d, B, np.zeros_like(B), MAX_ITER, _tol(dt), precond_diag=_diag(ip, ix, d) if pc else None)
    return _ref_cache[key]


def _pick(k):
    """The columns of a k-block: the rhs, uniform columns, and (k >= 3) the unit vector last."""
    return [0] if k == 1 else list(range(k - 1)) + [8]


def _solve(s, P, B, X, max_iter, tol):
    return s.precond_solve(P, B, X, max_iter, tol) if P is not None else s.solve(B, X, max_iter, tol)


def _true_res(ip, ix, d, b, x):
    import scipy.sparse as sp
    wide = np.complex128 if d.dtype.kind == "c" else np.float64
    n = ip.size - 1
    M = sp.csr_matrix((d.astype(wide), ix, ip), shape=(n, n))
    return np.linalg.norm(b.astype(wide) - M @ x.astype(wide)) / np.linalg.norm(b.astype(wide))


def _assert_columns(dt, pc, k, sel, system, got, checker):
    """Every column of one solve against the checker's: status, iteration count, residuals, solution."""
    (ip, ix, d, B), (its, res, st, X), (cits, cres, cX) = system, got, checker
    tol = _tol(dt)
    for j, c in enumerate(sel):
        err = np.max(np.abs(X[:, j] - cX[:, c])); true = _true_res(ip, ix, d, B[:, j], X[:, j])
        print("%s pc=%d k=%d col %d: its %d (checker %d) res %.3e (checker %.3e) true %.3e max|x - checker| %.3e"
              % (np.dtype(dt).name, pc, k, c, its[j], cits[c], res[j], cres[c], true, err))
        assert st[j] == ref.OK
        assert abs(int(its[j]) - int(cits[c])) <= max(5, int(cits[c]) // 4)
        assert res[j] <= tol and true <= 10 * tol                # test_gpu_cg.py's margin on the true residual
        if _is_single(dt):
            assert err < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        else:
            assert err <= 1e-7 * max(1.0, np.max(np.abs(cX[:, c])))
            if its[j] == cits[c]:                                # the same iteration: the same residual but for the sums' order
                assert np.isclose(res[j], cres[c], rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 1. against the checker
@pytest.mark.parametrize("k", [1, 3, 4, 8])
@pytest.mark.parametrize("pc", [False, True], ids=["none", "jacobi"])
@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_every_column_follows_the_checker(sa, dt, pc, k):
    ip, ix, d, Ball = _system(dt)
    n = Ball.shape[0]
    sel = _pick(k)
    B = np.ascontiguousarray(Ball[:, sel])
    cits, cres, cst, cX = _checker(dt, pc)
    assert np.all(cst == ref.OK) and 2 * cits.max() <= MAX_ITER
    A = sa.HipCsr.new((n, n), ip, ix, d)
    P = sa.DiagPrecond.new(_diag(ip, ix, d), t_dtype=d.dtype) if pc else None
    s = sa.CGMany.new(A, n, k)
    X = np.zeros((n, k), dt)
    its, res, st = _solve(s, P, B, X, MAX_ITER, _tol(dt))       # checker: at most 26 iterations
    _assert_columns(dt, pc, k, sel, (ip, ix, d, B), (its, res, st, X), (cits, cres, cX))
    assert s.last_status == 0


# ------------------------------------------------------------------------------------------------ 2. independence
@pytest.mark.parametrize("dt", [F64, C32], ids=lambda d: np.dtype(d).name)
def test_column_0_does_not_see_its_neighbours(sa, dt):
    ip, ix, d, Ball = _system(dt)
    n = Ball.shape[0]
    A = sa.HipCsr.new((n, n), ip, ix, d)
    s = sa.CGMany.new(A, n, 4)
    ctx = sa.default_ctx(0)
    out = []
    for sel, poll in (([0, 1, 2, 8], 16), ([0, 5, 6, 7], 16), ([0, 1, 2, 8], 1)):
        ctx.set("poll", poll)
        X = np.zeros((n, 4), dt)
        its, res, st = s.solve(np.ascontiguousarray(Ball[:, sel]), X, MAX_ITER, _tol(dt))     # checker: at most 26 iterations
        assert np.all(st == ref.OK)
        out.append((its, res, X))
    (i0, r0, X0), (i1, r1, X1), (i2, r2, X2) = out
    assert i0[0] == i1[0] and r0[0].tobytes() == r1[0].tobytes() and X0[:, 0].tobytes() == X1[:, 0].tobytes()
    assert np.array_equal(i0, i2) and r0.tobytes() == r2.tobytes() and X0.tobytes() == X2.tobytes()     # poll changes nothing


# ------------------------------------------------------------------------------------------------ 3. events
def test_events_of_one_solve(sa):
    """f64, k = 8: [rhs, zero, started at its solution, unit vector, NaN in the rhs, uniform 1..3] in one solve."""
    ip, ix, d, Ball = _system(F64)
    n = Ball.shape[0]
    tol = 1e-10
    exact = np.linalg.solve(ref.dense(ip, ix, d), Ball[:, 1])
    bad = Ball[:, 4].copy(); bad[n // 3] = np.nan
    B = np.stack([Ball[:, 0], np.zeros(n), Ball[:, 1], Ball[:, 8], bad, Ball[:, 2], Ball[:, 3], Ball[:, 5]], axis=1)
    X0 = np.zeros((n, 8)); X0[:, 1] = 1.0; X0[:, 2] = exact
    A = sa.HipCsr.new((n, n), ip, ix, d)
    s = sa.CGMany.new(A, n, 8)
    X = X0.copy()
    its, res, st = s.solve(B, X, MAX_ITER, tol)                   # checker: 26 iterations, the unit vector 20
    print("events: its", its, "status", st, "res", res)
    assert st[1] == ref.OK and its[1] == 0 and not np.any(X[:, 1])                    # zero right-hand side: x = 0
    assert st[2] == ref.OK and its[2] == 0 and res[2] <= tol and np.array_equal(X[:, 2], exact)    # converged at the start
    assert st[4] != ref.OK and s.last_status == st[4]             # the NaN column is the only one with an error
    ok = [0, 3, 5, 6, 7]
    assert np.all(st[ok] == ref.OK) and all(its[3] < its[j] for j in (0, 5, 6, 7))    # the unit vector stops first (20 against 26)
    # ... and without the NaN column every other column has the same bits
    B2 = B.copy(); B2[:, 4] = Ball[:, 4]
    X2 = X0.copy()
    its2, res2, st2 = s.solve(B2, X2, MAX_ITER, tol)
    keep = [0, 1, 2, 3, 5, 6, 7]
    assert np.all(st2 == ref.OK) and s.last_status == 0
    assert np.array_equal(its[keep], its2[keep]) and res[keep].tobytes() == res2[keep].tobytes()
    assert np.ascontiguousarray(X[:, keep]).tobytes() == np.ascontiguousarray(X2[:, keep]).tobytes()
    # the unit vector's x was frozen at its event: a solve stopped there leaves the same bits
    X3 = X0.copy()
    its3, _, st3 = s.solve(B2, X3, int(its[3]), tol)
    assert st3[3] == ref.OK and its3[3] == its[3] and X3[:, 3].tobytes() == X[:, 3].tobytes()
    assert all(st3[j] == ref.INSUFFICIENT_ITER and its3[j] == its[3] for j in (0, 5, 6, 7))
    # max_iter = 21: the unit vector (20 iterations) is done, the others (26) are not
    X4 = X0.copy()
    its4, _, st4 = s.solve(B2, X4, 21, tol)
    assert st4[3] == ref.OK and its4[3] == its[3]
    assert all(st4[j] == ref.INSUFFICIENT_ITER and its4[j] == 21 for j in (0, 4, 5, 6, 7))
    assert st4[1] == ref.OK and st4[2] == ref.OK and s.last_status == ref.INSUFFICIENT_ITER
    # a Jacobi diagonal with one negative entry: InvalidPreconditioner on a column that sees it
    dg = _diag(ip, ix, d); dg[n // 2 + 3] = -dg[n // 2 + 3]
    P = sa.DiagPrecond.new(dg, t_dtype=d.dtype)
    X5 = np.zeros((n, 8))
    its5, res5, st5 = s.precond_solve(P, B2, X5, MAX_ITER, tol)
    o = ref.cg(ip, ix, d, B2[:, 0].copy(), np.zeros(n), MAX_ITER, tol, precond_diag=dg)
    print("negative Jacobi entry: status", st5, "its", its5, "checker", o.status, o.its)
    assert o.status == ref.INVALID_PRECOND
    assert st5[0] == ref.INVALID_PRECOND and its5[0] == o.its and res5[0] < 0 and st5[1] == ref.OK


# ------------------------------------------------------------------------------------------------ 4. entry points
@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_entry_points(sa, dt):
    ip, ix, d, Ball = _system(dt)
    n = Ball.shape[0]
    tol = _tol(dt)
    A = sa.HipCsr.new((n, n), ip, ix, d)
    s = sa.CGMany.new(A, n, 8)
    B = np.ascontiguousarray(Ball[:, [0, 1, 8]])                  # k = 3 on a handle made for 8
    X = np.zeros((n, 3), dt)
    its, res, st = s.solve(B, X, MAX_ITER, tol)                   # checker: at most 26 iterations
    cits = _checker(dt, False)[0][[0, 1, 8]]
    assert np.all(st == ref.OK) and np.all(np.abs(its - cits) <= 5)
    dB, dX = sa.DevVec.from_numpy(B.ravel()), sa.DevVec.from_numpy(np.zeros(n * 3, dt))
    its_d, res_d, st_d = s.solve(dB, dX, MAX_ITER, tol)
    assert np.array_equal(its, its_d) and res.tobytes() == res_d.tobytes() and np.array_equal(st, st_d)
    assert dX.to_numpy().tobytes() == X.tobytes()
    # refusals: more columns than the handle carries, sizes, k outside 1..8 at creation; nothing is written
    s4 = sa.CGMany.new(A, n, 2)
    Xk = np.full((n, 3), 3, dt)
    with pytest.raises(ValueError):
        s4.solve(B, Xk, MAX_ITER, tol)
    assert np.all(Xk == 3)
    from sprsolve_amd.error import IncompatibleMatrixFormat
    with pytest.raises(IncompatibleMatrixFormat):
        s.solve(B[:-1], np.zeros((n, 3), dt), MAX_ITER, tol)
    with pytest.raises(IncompatibleMatrixFormat):
        s.solve(B, np.zeros((n - 1, 3), dt), MAX_ITER, tol)
    for k in (0, 9):
        with pytest.raises(ValueError):
            sa.CGMany.new(A, n, k)


# ------------------------------------------------------------------------------------------------ 5. the grid walk's knobs
@pytest.mark.parametrize("dt,pc,k", [(F64, False, 8), (C64, True, 3), (F32, False, 3)], ids=["float64-k8", "complex128-k3-jacobi", "float32-k3"])
def test_walk_knobs_change_nothing_but_the_sums_order(sa, dt, pc, k):
    """The batched functors under fused_kernel's two walks (knob ew_chunk) and two cache policies (stream_nt), on every pack width:
    f64 k = 8: 2-wide packs, 8 000 of them, so the eighth XCD's chunk of 1 024 is cut short; c64 k = 3 with Jacobi: 1-wide packs,
    kp = 4 with a padding column, 6 000 packs; f32 k = 3: 4-wide packs, one pack is one padded row.  stream_nt changes the cache
    policy alone: bit-identical results.  ew_chunk regroups the partials: each run meets the checker as in section 1."""
    ip, ix, d, Ball = _system(dt)
    n = Ball.shape[0]
    sel = _pick(k)
    B = np.ascontiguousarray(Ball[:, sel])
    cits, cres, cst, cX = _checker(dt, pc)
    assert np.all(cst == ref.OK)
    A = sa.HipCsr.new((n, n), ip, ix, d)
    P = sa.DiagPrecond.new(_diag(ip, ix, d), t_dtype=d.dtype) if pc else None
    s = sa.CGMany.new(A, n, k)
    ctx = sa.default_ctx(0)
    knobs = {name: ctx.get(name) for name in ("ew_chunk", "stream_nt")}
    try:
        for chunk in (0, 1):
            runs = []
            for nt in (0, 1):
                ctx.set("ew_chunk", chunk); ctx.set("stream_nt", nt)
                X = np.zeros((n, k), dt)
                its, res, st = _solve(s, P, B, X, MAX_ITER, _tol(dt))
                print("ew_chunk=%d stream_nt=%d" % (chunk, nt))
                _assert_columns(dt, pc, k, sel, (ip, ix, d, B), (its, res, st, X), (cits, cres, cX))
                assert s.last_status == 0
                runs.append((np.asarray(its).tobytes(), np.asarray(res).tobytes(), np.asarray(st).tobytes(), X.tobytes()))
            assert runs[0] == runs[1]
    finally:
        for name, value in knobs.items():
            ctx.set(name, value)
