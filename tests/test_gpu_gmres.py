"""Restarted GMRES on the GPU (sprs_gmres_*, csrc/gmres_fuse.hpp) against the numpy restatement of its recurrence
(tests/_gmres_ref.py): literal mode against the checker, the fused cycles against literal mode, the events of the recurrence,
every SpMV route, the entry points, the distributed operator at world 1 and one mid-size non-symmetric banded system through
the non-temporal flavour of the kernels.

The checker's step counts (x0 = 0; f64 / c64 at tol 1e-10, f32 / c32 at 1e-5; tests/test_gmres_cpu.py::COUNTS holds and
checks them) are, as f64 = c64 / f32 = c32:
    cd24x20  m = 1: 577 / 310   4: 133 / 77   5: 111 / 73   8: 125 / 77   9: 119 / 70   30: 136 / 65   64: 99 / 52
    cd64x48  m = 5: 221 / 161   30: 328 / 199
    tri1000  m = 5: 20 / 10 (Jacobi 19 / 9)   30: 20 / 10 (Jacobi 18 / 9)
Every max_iter is at least twice its count.  GmDots takes 8 basis vectors a launch (4 for c64), so m = 4, 5, 8, 9 straddle
its chunk boundary in every scalar type.

Trace rows are compared over the first 40 steps, across the restarts (15 on tri1000 with m = 5: test_gmres_cpu.py::trace_rows);
test_gmres_cpu.py::_self_check shows that the checker itself, with its sums reordered, holds a tenth of rtol 1e-9 / atol 1e-12
there, and res, x and the step count over the whole solve."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gmres_ref as ref  # noqa: E402
from test_gmres_cpu import COUNTS, diag_of, gpu_system, is_single, trace_close, trace_rows  # noqa: E402

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
_KNOBS = ("spmv_dict", "spmv_tile", "spmv_chain", "spmv_wide", "stream_nt")


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
    halo = ctx.get("halo_overlap")
    yield
    for k in _KNOBS:
        ctx.set(k, -1)
    ctx.set("halo_overlap", halo); ctx.set("poll", poll)


def _tol(dt):
    return 1e-5 if is_single(dt) else 1e-10


def _real_dtype(dt):
    return np.dtype(F32 if is_single(dt) else F64)


def _precond(sa, ip, ix, d, kind):
    """-> (DiagPrecond or None, the diagonal for the checker)."""
    if kind == "none":
        return None, None
    dg = diag_of(ip, ix, d)
    if kind == "jacobi":                                     # real V (DiagPrecond<T, T::Real>)
        dg = dg.real.astype(_real_dtype(d.dtype)).copy()
        return sa.DiagPrecond.new(dg, t_dtype=d.dtype), dg
    return sa.DiagPrecond.new(np.ascontiguousarray(dg)), dg  # complex V


def _true_res(ip, ix, d, rhs, x):
    wide = np.complex128 if rhs.dtype.kind == "c" else np.float64
    A = ref._matvec(ip, ix, d.astype(wide))
    return np.linalg.norm(rhs.astype(wide) - A(x.astype(wide))) / np.linalg.norm(rhs.astype(wide))


def _run(sa, solver, P, rhs, x, max_iter, tol):
    """-> (status, its, res) with the checker's status codes; x is updated in place."""
    E = sa.error
    try:
        its, res = solver.precond_solve(P, rhs, x, max_iter, tol) if P is not None else solver.solve(rhs, x, max_iter, tol)
        return ref.OK, its, res
    except E.InsufficientIterNum as e:
        return ref.INSUFFICIENT_ITER, e.iters, None
    except E.BreakDown as e:
        return ref.BREAKDOWN, e.its, None


def _margin(its):
    return max(5, its // 4)                                  # test_gpu_cg.py's


def _count(name, m, pc, dt):
    return COUNTS[(name, m, pc != "none")][ALL.index(dt)]


@functools.lru_cache(maxsize=None)
def _checker(name, m, pc, dtname):
    dt = np.dtype(dtname).type
    ip, ix, d, rhs = gpu_system(name, dt)
    dg = None
    if pc == "jacobi":
        dg = diag_of(ip, ix, d).real.astype(_real_dtype(dt)).copy()
    elif pc == "jacobi_complex":
        dg = diag_of(ip, ix, d)
    o = ref.gmres(ip, ix, d, rhs, np.zeros(rhs.size, dt), 2 * _count(name, m, pc if pc != "jacobi_complex" else "jacobi", dt), _tol(dt), restart=m, precond_diag=dg)
    o.x.setflags(write=False)
    return o


CASES = ([("cd24x20", m, "none") for m in (1, 4, 5, 8, 9, 30, 64)] + [("cd64x48", 5, "none"), ("cd64x48", 30, "none")]
         + [("tri1000", m, pc) for m in (5, 30) for pc in ("none", "jacobi")])
_ids = lambda v: v if isinstance(v, str) else (str(v) if isinstance(v, int) else np.dtype(v).name)


def _solve(sa, name, m, pc, dt, mode, trace=True, poll=None):
    ip, ix, d, rhs = gpu_system(name, dt)
    n = rhs.size
    P, _ = _precond(sa, ip, ix, d, pc)
    max_iter = 2 * _count(name, m, pc if pc != "jacobi_complex" else "jacobi", dt)
    if poll is not None:
        sa.default_ctx(0).set("poll", poll)
    A = sa.HipCsr.new((n, n), ip, ix, d)
    s = sa.GMRES.new(A, n, m); s.set_mode(mode)
    if trace:
        s.set_trace(max_iter)
    x = np.zeros(n, dt)
    st, its, res = _run(sa, s, P, rhs, x, max_iter, _tol(dt))
    return st, its, res, x, s.trace(), _true_res(ip, ix, d, rhs, x)


# ------------------------------------------------------------------------------------------------ 1. literal vs the checker
@pytest.mark.parametrize("name,m,pc,dt", [c + (dt,) for c in CASES for dt in ALL] + [("tri1000", 5, "jacobi_complex", C64), ("tri1000", 5, "jacobi_complex", C32)], ids=_ids)
def test_literal_follows_the_checker(sa, name, m, pc, dt):
    o = _checker(name, m, pc, np.dtype(dt).name)
    tol = _tol(dt)
    st, its, res, x, tr, true_res = _solve(sa, name, m, pc, dt, "literal")
    want = ref.trace_array(o.trace)
    err = np.max(np.abs(x - o.x))
    print("literal %s m=%d %s %s: its %d (checker %d) res %.3e (checker %.3e) true %.3e max|x - checker| %.3e rows %d"
          % (name, m, pc, np.dtype(dt).name, its, o.its, res, o.res, true_res, err, tr.shape[0]))
    assert st == o.status == ref.OK
    assert abs(its - o.its) <= _margin(o.its)
    assert tr.shape == (its, 8) and np.array_equal(tr[:, 0], np.arange(1, its + 1))
    assert res <= tol and true_res <= 10 * tol
    k = min(trace_rows(name, m), its, o.its)
    if is_single(dt):
        assert trace_close(tr[:1], want[:1], rtol=1e-5, atol=1e-8)
        assert err < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
    else:
        assert trace_close(tr[:k], want[:k], rtol=1e-9, atol=1e-12)
        assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
        assert its == o.its and np.isclose(res, o.res, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 2. fused vs literal
@pytest.mark.parametrize("dt", ALL, ids=_ids)
@pytest.mark.parametrize("name,m,pc", CASES, ids=_ids)
def test_fused_follows_literal(sa, name, m, pc, dt):
    tol = _tol(dt)
    sl, il, rl, xl, tl, _ = _solve(sa, name, m, pc, dt, "literal")
    sf, itf, rf, xf, tf, true_res = _solve(sa, name, m, pc, dt, "fused")
    print("fused %s m=%d %s %s: its %d (literal %d) res %.3e true %.3e max|dx| %.3e" % (name, m, pc, np.dtype(dt).name, itf, il, rf, true_res, np.max(np.abs(xf - xl))))
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert rf <= tol and true_res <= 10 * tol
    assert tf.shape == (itf, 8) and np.array_equal(tf[:, 0], np.arange(1, itf + 1))
    k = min(trace_rows(name, m), itf, il)
    if is_single(dt):
        assert np.max(np.abs(xf - xl)) < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert trace_close(tf[:1], tl[:1], rtol=1e-5, atol=1e-8)
    else:
        assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
        assert trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)               # the same scalars, step by step, across the restarts
        assert itf == il and np.isclose(rf, rl, rtol=1e-9, atol=1e-12)
    # late polling must not run the recurrence on: poll = 1 and poll = 16 give the same bits (no trace buffer: lazy polling)
    a = _solve(sa, name, m, pc, dt, "fused", trace=False, poll=1)
    b = _solve(sa, name, m, pc, dt, "fused", trace=False, poll=16)
    assert a[:3] == b[:3] == (sf, itf, rf) and np.array_equal(a[3], b[3]) and np.array_equal(a[3], xf)


# ------------------------------------------------------------------------------------------------ 3. events
def test_events_land_where_the_recurrence_says(sa):
    ip, ix, d, rhs = gpu_system("cd24x20", F64)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    exact = np.linalg.solve(ref.dense(ip, ix, d), rhs)
    for mode in ("fused", "literal"):
        s = sa.GMRES.new(A, n, 5); s.set_mode(mode)
        x = np.full(n, 3.0)
        assert _run(sa, s, None, np.zeros(n), x, 100, 1e-10) == (ref.OK, 0, 0.0) and not np.any(x), mode
        x = exact.copy()
        st, its, res = _run(sa, s, None, rhs, x, 100, 1e-10)
        assert (st, its) == (ref.OK, 0) and 0 <= res <= 1e-10 and np.array_equal(x, exact), mode
        for max_iter in (2, 10):                             # inside a cycle; exactly at a cycle's end
            x = np.zeros(n)
            assert _run(sa, s, None, rhs, x, max_iter, 1e-10)[:2] == (ref.INSUFFICIENT_ITER, max_iter), mode
            o = ref.gmres(ip, ix, d, rhs, np.zeros(n), max_iter, 1e-10, restart=5)
            assert o.status == ref.INSUFFICIENT_ITER and np.max(np.abs(x - o.x)) <= 1e-12 * np.max(np.abs(o.x)), (mode, max_iter)
        x = np.zeros(n)
        assert _run(sa, s, None, rhs, x, 0, 1e-10)[:2] == (ref.INSUFFICIENT_ITER, 0) and not np.any(x), mode
        bad = rhs.copy(); bad[n // 3] = np.nan
        st, its, _ = _run(sa, s, None, bad, np.zeros(n), 8, 1e-10)
        assert (st, its) == (ref.BREAKDOWN, 0), (mode, st, its)          # hn is NaN at the first step
        for bad_rhs, bad_x, code in ((rhs[:-1], np.zeros(n), "Input vec dimension"), (rhs, np.zeros(n + 1), "Input and output vec")):
            with pytest.raises(sa.error.IncompatibleMatrixFormat, match=code):
                s.solve(bad_rhs, bad_x, 10, 1e-10)
    with pytest.raises(ValueError):
        sa.GMRES.new(A, n, 65)
    assert sa.GMRES.new(A, n, 0).restart == 30 and sa.GMRES.new(A, n, 64).restart == 64
    # a preconditioner of the wrong size / scalar type
    with pytest.raises(sa.error.DimensionMismatch):
        sa.GMRES.new(A, n).precond_solve(sa.DiagPrecond.new(np.ones(3)), rhs, np.zeros(n), 10, 1e-10)
    with pytest.raises(ValueError):
        sa.GMRES.new(A, n).precond_solve(sa.DiagPrecond.new(np.ones(n), t_dtype=C64), rhs, np.zeros(n), 10, 1e-10)


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_tiny_systems(sa, dt):
    """n = 1 (hn == 0 at the first step) and n = 3 with m = 5 (the Krylov space is exhausted before the cycle is)."""
    from sprsolve_amd import gen
    tol = _tol(dt)
    for n in (1, 3):
        if n == 1:
            ip, ix, d, rhs = np.array([0, 1], np.int32), np.array([0], np.int32), np.array([4.0]), np.array([2.0])
        else:
            ip, ix, d, rhs = gen.random_tridiagonal(n)
        d = d.astype(dt); rhs = rhs.astype(dt)
        o = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), 20, tol, restart=5)
        assert o.status == ref.OK and 1 <= o.its <= n
        A = sa.HipCsr.new((n, n), ip, ix, d)
        for mode in ("fused", "literal"):
            s = sa.GMRES.new(A, n, 5); s.set_mode(mode)
            x = np.zeros(n, dt)
            st, its, res = _run(sa, s, None, rhs, x, 20, tol)
            assert st == ref.OK and 1 <= its <= n + 1 and res <= tol, (n, mode, its, res)
            assert _true_res(ip, ix, d, rhs, x) <= 10 * tol, (n, mode)
            assert np.allclose(x, o.x, rtol=1e-4 if is_single(dt) else 1e-9), (n, mode)


# ------------------------------------------------------------------------------------------------ 4. every SpMV route
def test_every_spmv_route(sa):
    """The plain stream, the offset codes and the pair codes, forced with "spmv_dict" on the 64 x 48 grid (its five offsets
    and five values qualify for both dictionaries)."""
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = gpu_system("cd64x48", F64)
    n = rhs.size
    want = _count("cd64x48", 30, "none", F64)
    runs = []
    for fmt in (0, 1, 2):
        ctx.set("spmv_dict", fmt)
        A = sa.HipCsr.new((n, n), ip, ix, d)
        r = A.spmv_route()
        assert r["format"] == fmt == A.stream_format()[0], (fmt, r)
        s = sa.GMRES.new(A, n, 30)
        x = np.zeros(n)
        st, its, res = _run(sa, s, None, rhs, x, 2 * want, 1e-10)
        print("route %d: kernel %s grid %d its %d res %.3e true %.3e" % (fmt, r["kernel"], r["grid"], its, res, _true_res(ip, ix, d, rhs, x)))
        assert st == ref.OK and _true_res(ip, ix, d, rhs, x) <= 10 * 1e-10
        runs.append((its, x))
    for its, x in runs[1:]:                                  # y is bit-identical on every route and GMRES takes no dot from the SpMV
        assert abs(its - runs[0][0]) <= 1 and np.max(np.abs(x - runs[0][1])) <= 1e-12 * np.max(np.abs(runs[0][1]))


# ------------------------------------------------------------------------------------------------ 5. entry points
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_device_and_host_entry_points_agree(sa, dt):
    ip, ix, d, rhs = gpu_system("tri1000", dt)
    n = rhs.size
    P, _ = _precond(sa, ip, ix, d, "jacobi")
    A = sa.HipCsr.new((n, n), ip, ix, d)
    s = sa.GMRES.new(A, n, 5)
    for pc in (None, P):
        x = np.zeros(n, dt)
        first = _run(sa, s, pc, rhs, x, 60, _tol(dt))                            # checker: at most 20 steps
        assert first[0] == ref.OK and first[1] > 5
        x2 = np.zeros(n, dt)
        assert _run(sa, s, pc, rhs, x2, 60, _tol(dt)) == first and np.array_equal(x2, x)        # workspace reuse
        d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
        assert _run(sa, s, pc, d_rhs, d_x, 60, _tol(dt)) == first
        assert np.array_equal(d_x.to_numpy(), x)


# ------------------------------------------------------------------------------------------------ 6. distributed operator
@pytest.mark.parametrize("with_halo", ["none", "tail-overlapped"])
def test_distributed_operator_world_1(sa, with_halo):
    import torch
    from sprsolve_amd import dist as sdist, gen
    from test_gpu_dist import _self_halo_plan
    ctx = sa.default_ctx(0)
    dev = torch.device("cuda", 0)
    comm = sdist.Comm(ctx, 0, 1)
    try:
        R = 96
        n = R * R
        ip, ix, d, rhs = gen.convection_diffusion_2d(R, R)
        mask = (lambda c: np.zeros(c.shape, bool)) if with_halo == "none" else (lambda c: c > n - 3 * R)
        plan = _self_halo_plan(torch, dev, n, ix, mask)
        assert (plan["n_ext"] > n) == (with_halo != "none")
        ctx.set("spmv_wide", 0)                              # the plain handle on the 64-row kernels of the subset launches
        A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip).to(dev), torch.from_numpy(d).to(dev), adopt=True,
                                    to_device=lambda a: torch.from_numpy(a).to(dev))
        plain = sa.HipCsr.new((n, n), ip, ix, d)
        P = sa.DiagPrecond.new(diag_of(ip, ix, d))
        for pc in (None, P):
            outs = []
            for op in (plain, A):
                s = sa.GMRES.new(op, n, 30)
                xs = torch.zeros(n, dtype=torch.float64, device=dev)
                st, its, res = _run(sa, s, pc, torch.from_numpy(rhs).to(dev), xs, 1000, 1e-8)    # checker: 473 steps
                outs.append((st, its, res, xs.cpu().numpy()))
            (s0, i0, r0, x0), (s1, i1, r1, x1) = outs
            rel = np.max(np.abs(x0 - x1)) / np.max(np.abs(x0))
            print("dist %s pc=%s: status %d / %d its %d / %d rel %.3e" % (with_halo, pc is not None, s0, s1, i0, i1, rel))
            assert s0 == s1 == ref.OK and abs(i0 - i1) <= 1 and rel <= 1e-12
            assert _true_res(ip, ix, d, rhs, x1) <= 1e-7
    finally:
        ctx.set("spmv_wide", -1)
        comm.close()


# ------------------------------------------------------------------------------------------------ 7. a mid-size banded system
def test_nonsymmetric_banded_through_the_nontemporal_kernels(sa):
    """cfg 3's banded matrix with its strict upper triangle halved.  A vector that crosses the 72 MB of the automatic
    non-temporal threshold needs 9.4 M rows, whose generation alone costs this test its few seconds; "stream_nt" = 1 sends
    200 000 rows through the NT = true flavour of every fused kernel instead, and the same solve with "stream_nt" = 0 must
    return the same bits."""
    from sprsolve_amd import gen
    ctx = sa.default_ctx(0)
    n = 200_000
    ip, ix, d, rhs = gen.symmetric_banded(n)
    rows = np.repeat(np.arange(n), np.diff(ip))
    d = np.where(ix > rows, 0.5 * d, d)
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n), 80, 1e-10, restart=30)
    assert o.status == ref.OK and 2 * o.its <= 80
    A = sa.HipCsr.new((n, n), ip, ix, d)
    got = []
    for nt in (1, 0):
        ctx.set("stream_nt", nt)
        s = sa.GMRES.new(A, n, 30)
        x = np.zeros(n)
        got.append(_run(sa, s, None, rhs, x, 80, 1e-10) + (x,))
    st, its, res, x = got[0]
    print("banded nt: its %d (checker %d) res %.3e true %.3e" % (its, o.its, res, _true_res(ip, ix, d, rhs, x)))
    assert st == ref.OK and abs(its - o.its) <= _margin(o.its) and res <= 1e-10
    assert _true_res(ip, ix, d, rhs, x) <= 1e-9
    assert np.max(np.abs(x - o.x)) <= 1e-7 * np.max(np.abs(o.x))
    assert got[1][:3] == got[0][:3] and np.array_equal(got[1][3], x)
