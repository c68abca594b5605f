"""LSMR on the GPU (sprs_lsmr_*, csrc/lsmr.hip, lsmr_fuse.hpp) against the numpy restatement of its recurrence
(tests/_lsmr_ref.py): literal mode against the checker, the fused five-launch iteration against literal mode, the events of
the recurrence and the entry points.

The checker's iteration counts from x = 0 on ref.system(m, n, dtype, seed = m + n), consistent / inconsistent rhs (measured on
the CPU; f64 / c64 at tol 1e-10, f32 / c32 at 1e-5); MAX_ITER = 80 is at least twice every one of them:
    f64   130x67 20 / 20   67x130 19 / 19   500x500 25 / 25   600x400 28 / 28
    c128  130x67 22 / 22   67x130 21 / 21   500x500 30 / 31   600x400 32 / 32
    f32   130x67 11 / 11   67x130 10 / 10   500x500 12 / 12   600x400 13 / 14
    c64   130x67 12 / 12   67x130 11 / 11   500x500 15 / 15   600x400 15 / 16
The solution tolerance of a case is the checker's own |x - x_lstsq| / |x_lstsq| on that input times 10 (room for the summation
order of the reductions); the checker's error measured 1.7e-10 .. 1.2e-9 in f64 / c128 and 2.7e-5 .. 8.2e-5 in f32 / c64."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lsmr_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
SHAPES = [(130, 67), (67, 130), (500, 500), (600, 400)]
MAX_ITER = 80
_ids = lambda v: np.dtype(v).name if isinstance(v, type) else ("%dx%d" % v if isinstance(v, tuple) else str(v))


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
    poll = ctx.get("poll")
    yield
    ctx.set("spmv_dict", -1); ctx.set("poll", poll)


def _is_single(dt):
    return np.dtype(dt) in (np.dtype(F32), np.dtype(C32))


def _tol(dt):
    return 1e-5 if _is_single(dt) else 1e-10


def _wide(dt):
    return C64 if np.dtype(dt).kind == "c" else F64


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@functools.lru_cache(maxsize=None)
def _case(dt, shape, consistent, damp=0.0, seed=None):
    """One system with everything the tests compare against, computed once: the checker's run from x = 0, lstsq's solution and
    the solution tolerance (the checker's own error against lstsq times 10)."""
    m, n = shape
    ip, ix, d, b = ref.system(m, n, dt, seed=m + n if seed is None else seed, consistent=consistent)
    o = ref.lsmr(shape, ip, ix, d, b, np.zeros(n, dt), MAX_ITER, _tol(dt), damp=damp)
    D = ref.dense(m, n, ip, ix, d)
    bw = b.astype(D.dtype)
    if damp:
        xl = np.linalg.lstsq(np.vstack([D, damp * np.eye(n)]), np.concatenate([bw, np.zeros(n, D.dtype)]), rcond=None)[0]
    else:
        xl = np.linalg.lstsq(D, bw, rcond=None)[0]
    assert o.status == ref.OK and 2 * o.its <= MAX_ITER
    for a in (ip, ix, d, b, xl, o.x):
        a.setflags(write=False)
    return dict(ip=ip, ix=ix, d=d, b=b, o=o, D=D, xl=xl, xtol=10 * _rel(o.x, xl))


def _run(sa, s, rhs, x, max_iter, tol, damp=0.0):
    """-> (status, its, res, ares) with the checker's status codes; x is updated in place."""
    E = sa.error
    try:
        its, res, ares = s.solve(rhs, x, max_iter, tol, damp=damp)
        return ref.OK, its, res, ares
    except E.InsufficientIterNum as e:
        return ref.INSUFFICIENT_ITER, e.iters, None, None
    except E.BreakDown as e:
        return ref.BREAKDOWN, e.its, None, None
    except E.DimensionMismatch:
        return ref.DIM_MISMATCH, None, None, None
    except ValueError:
        return ref.INVALID_ARGUMENT, None, None, None


def _margin(its):
    return max(5, its // 4)                                  # __graft_entry__.smoke's


def _true_res(c, x):
    """|b - A x| / |b| and |A^H r| / (|A|_F |r|) in numpy from the returned x."""
    xw = x.astype(c["D"].dtype)
    r = c["b"].astype(c["D"].dtype) - c["D"] @ xw
    nr = np.linalg.norm(r)
    return nr / np.linalg.norm(c["b"]), np.linalg.norm(c["D"].conj().T @ r) / (np.linalg.norm(c["D"]) * nr)


def _checker_at(c, shape, its):
    """The checker's (res, ares) after `its` iterations from x = 0: its own result where it stopped there, else a run that is
    not allowed to stop before (tol = 0), from the trace row and the running |A| that row belongs to."""
    o = c["o"]
    if its == o.its:
        return o.res, o.ares
    t = ref.lsmr(shape, c["ip"], c["ix"], c["d"], c["b"], np.zeros(shape[1], c["d"].dtype), its, 0.0)
    assert t.status == ref.INSUFFICIENT_ITER and len(t.trace) == its
    _, normr, normar, _, _, normA = t.trace[-1]
    return normr / float(np.linalg.norm(c["b"])), normar / (normA * normr)


def _solver(sa, c, shape, mode, adjoint=None):
    A = sa.HipCsr.new(shape, c["ip"], c["ix"], c["d"])
    s = sa.LSMR.new(A, adjoint)
    s.set_mode(mode)
    return A, s


# ------------------------------------------------------------------------------------------------ 1. literal vs the checker
@pytest.mark.parametrize("consistent", [True, False], ids=["consistent", "inconsistent"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_literal_follows_the_checker(sa, dt, shape, consistent):
    c = _case(dt, shape, consistent)
    o, tol = c["o"], _tol(dt)
    A, s = _solver(sa, c, shape, "literal")
    x = np.zeros(shape[1], dt)
    st, its, res, ares = _run(sa, s, c["b"], x, MAX_ITER, tol)
    tres, tares = _true_res(c, x)
    err = _rel(x, c["xl"])
    print("literal %s %dx%d %s: its %d (checker %d) res %.3e (true %.3e) ares %.3e (true %.3e) |x - lstsq| %.3e (tolerance %.3e)"
          % (np.dtype(dt).name, shape[0], shape[1], consistent, its, o.its, res, tres, ares, tares, err, c["xtol"]))
    assert st == o.status
    assert abs(its - o.its) <= _margin(o.its)
    assert err <= c["xtol"]
    # the recurrence's estimates against the true residuals: they agree while they stand above the rounding floor of the
    # dtype (eps times the condition of the estimate); below it both are noise of that size
    # (the checker's own res is within 5e-4 of the true one in f32 / c64 and 2e-7 in f64 / c128, measured on the CPU)
    floor = 50 * np.finfo(dt).eps
    assert abs(res - tres) <= 1e-3 * tres + floor
    # ares divides by the running estimate of |A|, sqrt(sum alpha^2 + beta^2) so far: at most |A|_F and at least alpha_1 =
    # |A^H b| / |b| >= sigma_min, so the reported value lies between the true one and |A|_F / sigma_min times it
    # (the checker: 1.7 .. 5.9 times, with |A|_F / sigma_min = 13 .. 45): the sanity check
    hi = np.linalg.norm(c["D"]) / np.linalg.svd(c["D"], compute_uv=False)[-1]
    assert tares * (1 - 1e-2) - floor <= ares <= tares * hi * (1 + 1e-2) + floor
    # ... and the value itself against the checker's at the same iteration: a quotient of three recurrence scalars, each of
    # which the trace comparison below holds to 1e-9 / 1e-4, so three times that (the checker's own ares moves by 2.8e-14 in
    # f64 / c128 and 5.0e-6 in f32 / c64 when its norms are summed in another order, measured on the CPU); the same for res
    want_res, want_ares = _checker_at(c, shape, its)
    rtol = 3 * (1e-4 if _is_single(dt) else 1e-9)
    assert abs(ares - want_ares) <= rtol * want_ares
    assert abs(res - want_res) <= rtol * want_res


# ------------------------------------------------------------------------------------------------ 2. fused vs literal
@pytest.mark.parametrize("consistent", [True, False], ids=["consistent", "inconsistent"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_fused_follows_literal(sa, dt, shape, consistent):
    c = _case(dt, shape, consistent)
    tol = _tol(dt)
    out = {}
    for mode in ("literal", "fused"):
        A, s = _solver(sa, c, shape, mode)
        s.set_trace(MAX_ITER)
        x = np.zeros(shape[1], dt)
        out[mode] = _run(sa, s, c["b"], x, MAX_ITER, tol) + (x, s.trace())
    (st_l, its_l, res_l, ares_l, x_l, tr_l), (st_f, its_f, res_f, ares_f, x_f, tr_f) = out["literal"], out["fused"]
    print("fused %s %dx%d: its %d (literal %d) |x - lstsq| %.3e (tolerance %.3e) rows %d / %d"
          % (np.dtype(dt).name, shape[0], shape[1], its_f, its_l, _rel(x_f, c["xl"]), c["xtol"], tr_f.shape[0], tr_l.shape[0]))
    assert st_f == st_l == ref.OK
    assert abs(its_f - its_l) <= 1
    assert _rel(x_f, c["xl"]) <= c["xtol"]
    assert tr_f.shape[0] == its_f and tr_l.shape[0] == its_l
    k = min(its_f, its_l)
    # rows (its, |r|, |A^H r|, alpha, beta), relative to each row's own value: no absolute term
    # (the checker's columns move by at most 2.8e-14 in f64 / c128 and 5.4e-6 in f32 / c64 when its norms are summed in
    # another order, measured on the CPU, converged rows included)
    rtol = 1e-4 if _is_single(dt) else 1e-9
    a, b = tr_f[:k], tr_l[:k]
    assert np.array_equal(a[:, 0], b[:, 0])
    for col in (1, 2, 4, 6):
        worst = float(np.max(np.abs(a[:, col] - b[:, col]) / np.abs(b[:, col])))
        print("  column %d: largest relative difference %.3e (bound %.0e)" % (col, worst, rtol))
        assert np.allclose(a[:, col], b[:, col], rtol=rtol, atol=0), col
    assert not tr_f[:, (3, 5, 7)].any() and not tr_l[:, (3, 5, 7)].any()        # real scalars: the imaginary slots hold 0


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_fused_does_not_depend_on_poll(sa, dt):
    shape = (600, 400)
    c = _case(dt, shape, False)
    got = []
    for poll in (1, 16):
        sa.default_ctx(0).set("poll", poll)
        A, s = _solver(sa, c, shape, "fused")
        x = np.zeros(shape[1], dt)
        got.append(_run(sa, s, c["b"], x, MAX_ITER, _tol(dt)) + (x.tobytes(),))
    assert got[0] == got[1]


@pytest.mark.parametrize("dt,shape", [(F64, (500, 500)), (C32, (130, 67))], ids=_ids)
def test_profile_counts_the_products_that_ran(sa, dt, shape):
    """The SpMV profile of a solve that converges after `its` iterations: start's two products (A x, A^H u) and two an iteration.
    Fused, the host has enqueued whole polls, and the stop test of iteration `its` is taken by the first vector launch of the
    next one, behind that iteration's product by A: that product ran, the 2 (enq - its) - 1 after it returned at once and are
    kept out of the count.  With poll = 1 (and in literal mode) nothing is enqueued past the event."""
    c = _case(dt, shape, False)                               # checker: 25 / 12 iterations, so the last poll enqueues past the event
    got = {}
    for mode, poll in (("fused", 16), ("fused", 1), ("literal", 16)):
        sa.default_ctx(0).set("poll", poll)
        A, s = _solver(sa, c, shape, mode)
        s.set_profile(True)
        x = np.zeros(shape[1], dt)
        st, its, res, ares = _run(sa, s, c["b"], x, MAX_ITER, _tol(dt))
        p = s.profile()
        s.set_profile(False)
        print("profile %s %s poll %d: its %d steps %d launches %d" % (np.dtype(dt).name, mode, poll, its, p["steps"], p["spmv_launches"]))
        assert st == ref.OK
        enq = its if (mode == "literal" or poll == 1) else min(-(-its // 16) * 16, MAX_ITER)
        assert p["steps"] == 2 + 2 * enq
        assert p["spmv_launches"] == 2 + 2 * its + (1 if enq > its else 0)
        assert p["spmv_ms_total"] > 0 and p["solve_ms"] >= p["spmv_ms_total"]
        got[(mode, poll)] = (its, res, ares, x.tobytes())
    assert got[("fused", 16)] == got[("fused", 1)]            # and the profile changes no result


# ------------------------------------------------------------------------------------------------ 3. one case each
@pytest.mark.parametrize("mode", ["fused", "literal"])
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_minimum_norm(sa, dt, mode):
    shape = (67, 130)
    c = _case(dt, shape, True)
    A, s = _solver(sa, c, shape, mode)
    x = np.zeros(130, dt)
    st, its, res, _ = _run(sa, s, c["b"], x, MAX_ITER, _tol(dt))
    assert st == ref.OK and res <= 10 * _tol(dt)
    assert _rel(x, c["xl"]) <= c["xtol"]                     # lstsq returns the minimum-norm solution
    assert np.linalg.norm(x) <= np.linalg.norm(c["xl"]) * (1 + c["xtol"])


@pytest.mark.parametrize("mode", ["fused", "literal"])
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_damped(sa, dt, mode):
    shape, lam = (130, 67), 0.7
    c = _case(dt, shape, False, damp=lam, seed=5)            # checker: 18 / 20 / 9 / 11 iterations (f64 / c128 / f32 / c64)
    A, s = _solver(sa, c, shape, mode)
    x = np.zeros(67, dt)
    st, its, _, _ = _run(sa, s, c["b"], x, MAX_ITER, _tol(dt), damp=lam)
    assert st == ref.OK and abs(its - c["o"].its) <= _margin(c["o"].its)
    assert _rel(x, c["xl"]) <= c["xtol"]


@pytest.mark.parametrize("mode", ["fused", "literal"])
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_initial_guess(sa, dt, mode):
    shape = (130, 67)
    c = _case(dt, shape, False)
    x0 = (c["xl"] * (1 + 1e-2)).astype(dt)
    o = ref.lsmr(shape, c["ip"], c["ix"], c["d"], c["b"], x0, MAX_ITER, _tol(dt))
    assert o.status == ref.OK and o.its < c["o"].its
    A, s = _solver(sa, c, shape, mode)
    x = x0.copy()
    st, its, _, _ = _run(sa, s, c["b"], x, MAX_ITER, _tol(dt))
    assert st == ref.OK and abs(its - o.its) <= _margin(o.its)
    assert _rel(x, c["xl"]) <= max(c["xtol"], 10 * _rel(o.x, c["xl"]))


@pytest.mark.parametrize("mode", ["fused", "literal"])
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_events(sa, dt, mode):
    shape = (130, 67)
    c = _case(dt, shape, True)
    A, s = _solver(sa, c, shape, mode)
    tol = _tol(dt)
    # zero rhs: x = 0 whatever it held
    x = np.ones(67, dt)
    assert _run(sa, s, np.zeros(130, dt), x, MAX_ITER, tol)[:2] == (ref.OK, 0) and not x.any()
    # the iteration cap, with the reported count
    assert _run(sa, s, c["b"], np.zeros(67, dt), 3, tol)[:2] == (ref.INSUFFICIENT_ITER, 3)
    # a NaN in rhs
    bad = np.array(c["b"]); bad[5] = np.nan
    assert _run(sa, s, bad, np.zeros(67, dt), MAX_ITER, tol)[0] == ref.BREAKDOWN
    # lengths and damp
    assert _run(sa, s, c["b"][:-1], np.zeros(67, dt), MAX_ITER, tol)[0] == ref.DIM_MISMATCH
    assert _run(sa, s, c["b"], np.zeros(68, dt), MAX_ITER, tol)[0] == ref.DIM_MISMATCH
    assert _run(sa, s, c["b"], np.zeros(67, dt), MAX_ITER, tol, damp=-1.0)[0] == ref.INVALID_ARGUMENT
    # and the handle still solves
    x = np.zeros(67, dt)
    assert _run(sa, s, c["b"], x, MAX_ITER, tol)[0] == ref.OK and _rel(x, c["xl"]) <= c["xtol"]


@pytest.mark.parametrize("mode", ["fused", "literal"])
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_lucky_termination(sa, dt, mode):
    n = 8
    ip = np.arange(n + 1, dtype=np.int32); ix = np.arange(n, dtype=np.int32)
    d = (np.arange(n) + 2.0).astype(dt)
    b = np.zeros(n, dt); b[3] = 1.0
    A = sa.HipCsr.new((n, n), ip, ix, d)
    s = sa.LSMR.new(A); s.set_mode(mode)
    x = np.zeros(n, dt)
    st, its, res, ares = _run(sa, s, b, x, 10, _tol(dt))
    assert (st, its) == (ref.OK, 1)
    want = np.zeros(n, dt); want[3] = 1.0 / d[3]
    assert np.allclose(x, want, rtol=4 * np.finfo(dt).eps, atol=0)


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_entry_points_and_adjoint_handles_agree_on_bits(sa, dt):
    shape = (600, 400)
    c = _case(dt, shape, False)
    A, s = _solver(sa, c, shape, "fused")
    x_host = np.zeros(400, dt)
    r_host = _run(sa, s, c["b"], x_host, MAX_ITER, _tol(dt))
    bd = sa.DevVec.from_numpy(c["b"]); xd = sa.DevVec(400, dt); xd.zero()
    r_dev = _run(sa, s, bd, xd, MAX_ITER, _tol(dt))
    assert r_dev == r_host and xd.to_numpy().tobytes() == x_host.tobytes()
    AH = A.adjoint()
    s2 = sa.LSMR.new(A, AH)                                  # the caller's adjoint handle
    x2 = np.zeros(400, dt)
    assert _run(sa, s2, c["b"], x2, MAX_ITER, _tol(dt)) == r_host and x2.tobytes() == x_host.tobytes()
    with pytest.raises(sa.error.DimensionMismatch):
        sa.LSMR.new(A, A)                                    # not the adjoint's shape


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_cache_resident_stencil(sa, dt):
    """A 64 x 64 upwind grid (non-symmetric): the compressed stream on A and on its adjoint.  Checker: 27 iterations in f64 / c128
    at 1e-10, 11 in f32 / c64 at 1e-5 (measured on the CPU)."""
    import scipy.sparse as sp
    nx = 64
    e = np.ones(nx)
    Tx = sp.diags([-e[:-1], 1.5 * e], [-1, 0]); Ty = sp.diags([-0.5 * e[:-1], 1.5 * e], [-1, 0])
    M = (sp.kron(sp.eye(nx), Tx) + sp.kron(Ty, sp.eye(nx))).tocsr(); M.sort_indices()
    n = nx * nx
    ip, ix, d = M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(dt)
    xs = np.cos(np.arange(n) * 0.37).astype(dt)
    b = (M @ xs).astype(dt)
    tol, cap = _tol(dt), MAX_ITER
    o = ref.lsmr((n, n), ip, ix, d, b, np.zeros(n, dt), cap, tol)
    assert o.status == ref.OK and 2 * o.its <= cap
    A = sa.HipCsr.new((n, n), ip, ix, d)
    AH = A.adjoint()
    assert A.stream_format()[0] != 0 and AH.stream_format()[0] != 0
    s = sa.LSMR.new(A, AH)
    x = np.zeros(n, dt)
    st, its, res, _ = _run(sa, s, b, x, cap, tol)
    xw = np.linalg.solve(M.toarray().astype(_wide(dt)), b.astype(_wide(dt)))
    print("stencil %s: its %d (checker %d) |x - solve| %.3e (checker %.3e)" % (np.dtype(dt).name, its, o.its, _rel(x, xw), _rel(o.x, xw)))
    assert st == ref.OK and abs(its - o.its) <= _margin(o.its)
    assert _rel(x, xw) <= 10 * _rel(o.x, xw)


@pytest.mark.parametrize("dt", [F64, C32], ids=_ids)
def test_many_workgroups(sa, dt):
    """200 000 x 100 000: more than one workgroup in every kernel, i.e. the partials and their re-reduction.  No dense check at
    this size: the checker's x is the reference (its own error against lstsq on the small systems is in the module docstring)."""
    shape = (200000, 100000)
    ip, ix, d, b = ref.system(shape[0], shape[1], dt, seed=3, consistent=True)
    tol = _tol(dt)
    o = ref.lsmr(shape, ip, ix, d, b, np.zeros(shape[1], dt), MAX_ITER, tol)    # 20 iterations in f64, 11 in c64 (measured)
    assert o.status == ref.OK and 2 * o.its <= MAX_ITER
    A = sa.HipCsr.new(shape, ip, ix, d)
    s = sa.LSMR.new(A)
    x = np.zeros(shape[1], dt)
    st, its, res, ares = _run(sa, s, b, x, MAX_ITER, tol)
    print("large %s: its %d (checker %d) res %.3e (checker %.3e) |x - checker| %.3e" % (np.dtype(dt).name, its, o.its, res, o.res, _rel(x, o.x)))
    assert st == ref.OK and abs(its - o.its) <= _margin(o.its)
    assert _rel(x, o.x) <= 100 * tol                         # both stop at |r| <= tol (|b| + |A| |x|) on a system of condition < 4
