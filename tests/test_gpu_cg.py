"""Conjugate gradients on the GPU (sprs_cg_*, csrc/cg_fuse.hpp) against the numpy restatement of its recurrence
(tests/_cg_ref.py): literal mode against the checker, the fused three-launch iteration against literal mode, every SpMV
route, the events of the recurrence, the entry points, the distributed operator at world 1 and the BASELINE shapes.

The checker's iteration counts (x0 = 0; measured on the CPU with tests/_cg_ref.py; f64 / c64 at tol 1e-10, f32 / c32 at 1e-5)
stand beside every max_iter; each max_iter is at least twice its count."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
_KNOBS = ("spmv_dict", "spmv_tile", "spmv_chain", "spmv_wide", "halo_overlap")


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
    for k in _KNOBS[:4]:
        ctx.set(k, -1)
    ctx.set("halo_overlap", halo); ctx.set("poll", poll)


def _is_single(dt):
    return np.dtype(dt) in (np.dtype(F32), np.dtype(C32))


def _tol(dt):
    return 1e-5 if _is_single(dt) else 1e-10


def _system(dt):
    """The banded generators (their diagonal varies, so Jacobi is not a constant scaling) in the dtype under test."""
    from sprsolve_amd import gen
    if np.dtype(dt).kind == "c":
        ip, ix, d, rhs = gen.hermitian_banded(1500, 3)       # checker: 26 iterations (24 with Jacobi); c32: 13 (12)
    else:
        ip, ix, d, rhs = gen.symmetric_banded(2000)          # checker: 26 iterations (23 with Jacobi); f32: 14 (12)
    return ip, ix, d.astype(dt), rhs.astype(dt)


MAX_ITER = 80                                                # >= 2 * 26, the largest count of _system


def _diag(ip, ix, d):
    rows = np.repeat(np.arange(ip.size - 1), np.diff(ip))
    return d[rows == ix]


def _real_dtype(dt):
    return np.dtype(F32 if _is_single(dt) else F64)


def _precond(sa, ip, ix, d, kind):
    """-> (DiagPrecond or None, the diagonal for the checker)."""
    if kind == "none":
        return None, None
    dg = _diag(ip, ix, d)
    if kind == "jacobi":                                     # real V (DiagPrecond<T, T::Real>)
        dg = dg.real.astype(_real_dtype(d.dtype)).copy()
        return sa.DiagPrecond.new(dg, t_dtype=d.dtype), dg
    return sa.DiagPrecond.new(np.ascontiguousarray(dg)), dg  # complex V


def _matvec(ip, ix, d, v):
    import scipy.sparse as sp
    n = ip.size - 1
    return sp.csr_matrix((d.astype(np.complex128 if d.dtype.kind == "c" else np.float64), ix, ip), shape=(n, n)) @ v


def _true_res(ip, ix, d, rhs, x):
    rhs = rhs.astype(np.complex128 if rhs.dtype.kind == "c" else np.float64)
    return np.linalg.norm(rhs - _matvec(ip, ix, d, x.astype(rhs.dtype))) / np.linalg.norm(rhs)


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
    except E.InvalidPreconditioner as e:
        return ref.INVALID_PRECOND, None, e.msg


def _trace_close(a, b, rtol, atol=1e-8):
    """Trace rows compared as [its, r_norm, rho, alpha, beta] with rho, alpha, beta as the complex numbers they are: on a
    Hermitian system their imaginary parts are rounding noise of the size of eps * |value|, which no relative tolerance on
    the component alone can hold."""
    def cx(t):
        t = np.atleast_2d(t)
        return np.concatenate([t[:, :2].astype(complex), t[:, 2::2] + 1j * t[:, 3::2]], axis=1)
    return np.allclose(cx(a), cx(b), rtol=rtol, atol=atol)


def _margin(its):
    return max(5, its // 4)                                  # __graft_entry__.smoke's


# ------------------------------------------------------------------------------------------------ 1. literal vs the checker
@pytest.mark.parametrize("dt,pc", [(dt, pc) for dt in ALL for pc in ("none", "jacobi")] + [(C64, "jacobi_complex"), (C32, "jacobi_complex")],
                         ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_literal_follows_the_checker(sa, dt, pc):
    ip, ix, d, rhs = _system(dt)
    n = rhs.size
    P, dg = _precond(sa, ip, ix, d, pc)
    tol = _tol(dt)
    o = ref.cg(ip, ix, d, rhs, np.zeros(n, dt), MAX_ITER, tol, precond_diag=dg)
    assert o.status == ref.OK and 2 * o.its <= MAX_ITER
    A = sa.HipCsr.new((n, n), ip, ix, d)
    s = sa.CG.new(A, n); s.set_mode("literal"); s.set_trace(MAX_ITER)
    x = np.zeros(n, dt)
    st, its, res = _run(sa, s, P, rhs, x, MAX_ITER, tol)
    tr, want = s.trace(), ref.trace_array(o.trace)
    err = np.max(np.abs(x - o.x))
    print("literal %s %s: its %d (checker %d) res %.3e (checker %.3e) max|x - checker| %.3e rows %d" % (np.dtype(dt).name, pc, its, o.its, res, o.res, err, tr.shape[0]))
    assert (st, its) == (o.status, o.its)
    assert tr.shape == want.shape == (o.its - 1, 8)
    if _is_single(dt):
        # the tolerances of test_f32_solvers_against_oracle: first trace row to f32 rounding, x to 2e-3 (f32) / 5e-3 (c32)
        assert _trace_close(tr[0], want[0], rtol=1e-5)
        assert err < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert res <= tol
    else:
        assert _trace_close(tr, want, rtol=1e-9, atol=1e-12)
        assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
        assert np.isclose(res, o.res, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 2. fused vs literal
@pytest.mark.parametrize("pc", ["none", "jacobi"])
@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_fused_follows_literal(sa, dt, pc):
    ip, ix, d, rhs = _system(dt)
    n = rhs.size
    P, _ = _precond(sa, ip, ix, d, pc)
    tol = _tol(dt)
    A = sa.HipCsr.new((n, n), ip, ix, d)
    out = {}
    for mode in ("literal", "fused"):
        s = sa.CG.new(A, n); s.set_mode(mode); s.set_trace(MAX_ITER)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, MAX_ITER, tol)      # checker: at most 26 iterations
        out[mode] = (st, its, res, x, s.trace())
    (sl, il, rl, xl, tl), (sf, itf, rf, xf, tf) = out["literal"], out["fused"]
    true_res = _true_res(ip, ix, d, rhs, xf)
    print("fused %s %s: its %d (literal %d) res %.3e true %.3e max|dx| %.3e" % (np.dtype(dt).name, pc, itf, il, rf, true_res, np.max(np.abs(xf - xl))))
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert true_res <= 10 * tol
    if _is_single(dt):
        assert np.max(np.abs(xf - xl)) < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert _trace_close(tf[0], tl[0], rtol=1e-5)
    else:
        assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
        k = min(tf.shape[0], tl.shape[0])
        assert k >= il - 2 and _trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)      # the same scalars, iteration by iteration
    # without a trace buffer (lazy polling) the fused solve returns the same bits
    s = sa.CG.new(A, n)
    x2 = np.zeros(n, dt)
    assert _run(sa, s, P, rhs, x2, MAX_ITER, tol)[:2] == (sf, itf) and np.array_equal(x2, xf)
    prof = s.profile()
    assert prof["fused_k2"] == 0 and prof["fused_k4"] == 0


# ------------------------------------------------------------------------------------------------ 3. every SpMV route
def test_every_spmv_route(sa):
    """y is bit-identical on every route; what differs between routes is how the rows are grouped into the dot product's
    per-workgroup partials.  Routes that deal the same row blocks to the same grid in the same order give the same partials,
    hence the same x bit for bit: the plain stream and the offset codes (1024 workgroups, 7680 blocks of 64 rows).  Any other
    pair agrees to 1e-12.  Equal grids alone do not make equal partials: the pair-code stream on the same 1024 workgroups walks
    128-row blocks (3840 of them, two rows per lane) or, with "spmv_wide" = 0, its 64-row blocks in the far-band period order,
    and measured 8.0e-14 and 6.5e-14 relative from the plain stream after 274 iterations on every route."""
    from test_gpu_dict_stream import _chain_cases
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = _chain_cases()["p3_160x128x24"]()[:4]
    n = rhs.size
    tol, max_iter = 1e-10, 600                               # checker: 274 iterations
    configs = [("csr", dict(spmv_dict=0), 0, ("Csr", "CsrWide")),
               ("offsets", dict(spmv_dict=1), 1, ("Dict", "DictWide", "TileOff")),
               ("pairs", dict(spmv_dict=2), 2, ("Pair2", "TilePair")),
               ("chain", dict(spmv_dict=-1, spmv_tile=1, spmv_chain=1), 2, ("Chain",))]
    runs = []
    try:
        for label, knobs, fmt, kernels in configs:
            for k in ("spmv_dict", "spmv_tile", "spmv_chain", "spmv_wide"):
                ctx.set(k, knobs.get(k, -1))
            A = sa.HipCsr.new((n, n), ip, ix, d)
            r = A.spmv_route()
            assert r["format"] == fmt == A.stream_format()[0] and r["kernel"] in kernels, (label, r)
            if label == "chain":
                assert A.chain_plan()[0] >= 64, A.chain_plan()
            s = sa.CG.new(A, n)
            x = np.zeros(n)
            st, its, res = _run(sa, s, None, rhs, x, max_iter, tol)
            assert A.spmv_route() == r
            print("route %s: kernel %s grid %d its %d res %.3e true %.3e" % (label, r["kernel"], r["grid"], its, res, _true_res(ip, ix, d, rhs, x)))
            assert st == ref.OK and _true_res(ip, ix, d, rhs, x) <= 10 * tol
            runs.append((label, r, its, x))
    finally:
        for k in ("spmv_dict", "spmv_tile", "spmv_chain", "spmv_wide"):
            ctx.set(k, -1)
    checked_same = 0
    for i in range(len(runs)):
        for j in range(i + 1, len(runs)):
            (la, ra, ia, xa), (lb, rb, ib, xb) = runs[i], runs[j]
            same = np.array_equal(xa.view(np.uint64), xb.view(np.uint64))
            rel = np.max(np.abs(xa - xb)) / np.max(np.abs(xa))
            print("routes %s / %s: grids %d / %d, row blocks %d / %d, its %d / %d, bit-identical %s, rel %.3e"
                  % (la, lb, ra["grid"], rb["grid"], ra["n_blocks"], rb["n_blocks"], ia, ib, same, rel))
            assert abs(ia - ib) <= 1 and rel <= 1e-12, (la, lb)
            if ra["grid"] == rb["grid"] and ra["n_blocks"] == rb["n_blocks"] and ra["ordered"] == rb["ordered"] and 2 not in (ra["format"], rb["format"]):
                checked_same += 1
                assert same, (la, lb)
    assert checked_same >= 1


# ------------------------------------------------------------------------------------------------ 4. events
def test_events_land_where_the_recurrence_says(sa):
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = _system(F64)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    neg = sa.HipCsr.new((n, n), ip, ix, -d)
    for mode in ("fused", "literal"):
        s = sa.CG.new(neg, n); s.set_mode(mode)
        x = np.zeros(n)
        assert _run(sa, s, None, rhs, x, MAX_ITER, 1e-10)[:2] == (ref.BREAKDOWN, 0) and not np.any(x), mode
        s = sa.CG.new(A, n); s.set_mode(mode)
        x = np.zeros(n)
        assert _run(sa, s, None, rhs, x, 2, 1e-10)[:2] == (ref.INSUFFICIENT_ITER, 2), mode     # its_out == max_iter
        o = ref.cg(ip, ix, d, rhs, np.zeros(n), 2, 1e-10)
        assert np.max(np.abs(x - o.x)) <= 1e-12 * np.max(np.abs(o.x)), mode                      # two iterations were made, no more
        x = np.full(n, 3.0)
        assert _run(sa, s, None, np.zeros(n), x, MAX_ITER, 1e-10) == (ref.OK, 0, 0.0) and not np.any(x), mode
        exact = np.linalg.solve(ref.dense(ip, ix, d), rhs)
        x = exact.copy()
        st, its, res = _run(sa, s, None, rhs, x, MAX_ITER, 1e-10)
        assert (st, its) == (ref.OK, 0) and 0 <= res <= 1e-10 and np.array_equal(x, exact), mode
        for bad_rhs, bad_x, code in ((rhs[:-1], np.zeros(n), "Input vec dimension"), (rhs, np.zeros(n + 1), "Input and output vec")):
            with pytest.raises(sa.error.IncompatibleMatrixFormat, match=code):
                s.solve(bad_rhs, bad_x, 10, 1e-10)
    import ctypes as C
    from sprsolve_amd import _lib
    s = sa.CG.new(A, n)
    its = C.c_size_t(); res = C.c_double(); xb = np.zeros(n + 1)
    args = lambda r, rl, xx, xl: (s.h, r.ctypes.data_as(C.c_void_p), rl, xx.ctypes.data_as(C.c_void_p), xl, 10, 1e-10, C.byref(its), C.byref(res))
    assert _lib.lib().sprs_cg_solve_d(*args(rhs, n - 1, xb, n)) == 1
    assert _lib.lib().sprs_cg_solve_d(*args(rhs, n, xb, n + 1)) == 2
    # a Jacobi "preconditioner" with one negative entry on diag(1, 2, 3): the checker's case (tests/test_cg_cpu.py)
    ip3 = np.array([0, 1, 2, 3], np.int32); ix3 = np.array([0, 1, 2], np.int32); d3 = np.array([1.0, 2.0, 3.0])
    o = ref.cg(ip3, ix3, d3, np.ones(3), np.zeros(3), 10, 1e-12, precond_diag=np.array([1.0, 2.0, -3.0]))
    assert (o.status, o.its) == (ref.INVALID_PRECOND, 0)
    A3 = sa.HipCsr.new((3, 3), ip3, ix3, d3)
    P3 = sa.DiagPrecond.new(np.array([1.0, 2.0, -3.0]))
    for mode in ("fused", "literal"):
        s = sa.CG.new(A3, 3); s.set_mode(mode)
        x = np.zeros(3)
        with pytest.raises(sa.error.InvalidPreconditioner, match=r"beta_0 \[-0\.69421") as ei:
            s.precond_solve(P3, np.ones(3), x, 10, 1e-12)
        assert np.allclose(x, o.x, rtol=1e-14), (mode, ei.value)
    # a preconditioner of the wrong size / scalar type
    with pytest.raises(sa.error.DimensionMismatch):
        sa.CG.new(A, n).precond_solve(P3, rhs, np.zeros(n), 10, 1e-10)
    with pytest.raises(ValueError):
        sa.CG.new(A, n).precond_solve(sa.DiagPrecond.new(np.ones(n), t_dtype=C64), rhs, np.zeros(n), 10, 1e-10)
    # late polling must not run the recurrence on
    got = []
    try:
        for poll in (1, 7, 64):
            ctx.set("poll", poll)
            s = sa.CG.new(A, n)
            x = np.zeros(n)
            got.append(_run(sa, s, None, rhs, x, MAX_ITER, 1e-10) + (x,))       # checker: 26 iterations
    finally:
        ctx.set("poll", 16)
    assert got[0][0] == ref.OK and got[0][1] == 26
    for g in got[1:]:
        assert g[:3] == got[0][:3] and np.array_equal(g[3].view(np.uint64), got[0][3].view(np.uint64))


# ------------------------------------------------------------------------------------------------ 5. entry points
@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_device_and_host_entry_points_agree(sa, dt):
    ip, ix, d, rhs = _system(dt)
    n = rhs.size
    P, _ = _precond(sa, ip, ix, d, "jacobi")
    A = sa.HipCsr.new((n, n), ip, ix, d)
    s = sa.CG.new(A, n)
    for pc in (None, P):
        x = np.zeros(n, dt)
        first = _run(sa, s, pc, rhs, x, MAX_ITER, _tol(dt))                      # checker: at most 26 iterations
        assert first[0] == ref.OK and first[1] > 5
        x2 = np.zeros(n, dt)
        assert _run(sa, s, pc, rhs, x2, MAX_ITER, _tol(dt)) == first and np.array_equal(x2, x)      # workspace reuse
        d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
        assert _run(sa, s, pc, d_rhs, d_x, MAX_ITER, _tol(dt)) == first
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
        n = 96 * 96
        ip, ix, d, rhs = gen.symmetric_banded(n)             # checker: 26 iterations (23 with Jacobi)
        mask = (lambda c: np.zeros(c.shape, bool)) if with_halo == "none" else (lambda c: c > n - 3 * 96)
        plan = _self_halo_plan(torch, dev, n, ix, mask)
        assert (plan["n_ext"] > n) == (with_halo != "none")
        ctx.set("spmv_wide", 0)                              # the plain handle on the 64-row kernels of the subset launches
        A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip).to(dev), torch.from_numpy(d).to(dev), adopt=True,
                                    to_device=lambda a: torch.from_numpy(a).to(dev))
        plain = sa.HipCsr.new((n, n), ip, ix, d)
        P = sa.DiagPrecond.new(_diag(ip, ix, d))
        for pc in (None, P):
            outs = []
            for op in (plain, A):
                s = sa.CG.new(op, n)
                xs = torch.zeros(n, dtype=torch.float64, device=dev)
                st, its, res = _run(sa, s, pc, torch.from_numpy(rhs).to(dev), xs, MAX_ITER, 1e-10)
                outs.append((st, its, res, xs.cpu().numpy()))
            (s0, i0, r0, x0), (s1, i1, r1, x1) = outs
            rel = np.max(np.abs(x0 - x1)) / np.max(np.abs(x0))
            print("dist %s pc=%s: its %d / %d rel %.3e" % (with_halo, pc is not None, i0, i1, rel))
            assert s0 == s1 == ref.OK and i0 == i1 and rel <= 1e-12
            assert _true_res(ip, ix, d, rhs, x1) <= 1e-9
    finally:
        ctx.set("spmv_wide", -1)
        comm.close()


# ------------------------------------------------------------------------------------------------ 7. non-finite input
def test_nan_in_rhs_ends_in_a_status(sa):
    ip, ix, d, rhs = _system(F64)
    n = rhs.size
    rhs = rhs.copy(); rhs[n // 3] = np.nan
    A = sa.HipCsr.new((n, n), ip, ix, d)
    for mode in ("fused", "literal"):
        s = sa.CG.new(A, n); s.set_mode(mode)
        st, its, _ = _run(sa, s, None, rhs, np.zeros(n), 8, 1e-10)
        assert (st, its) in ((ref.BREAKDOWN, 0), (ref.INSUFFICIENT_ITER, 8)), (mode, st, its)


# ------------------------------------------------------------------------------------------------ 8. BASELINE shapes
@pytest.mark.parametrize("pc", ["none", "jacobi"])
def test_cfg3_banded_full_size(sa, pc):
    from sprsolve_amd import gen
    n = 1_000_000
    ip, ix, d, rhs = gen.symmetric_banded(n)
    P, dg = _precond(sa, ip, ix, d, pc)
    o = ref.cg(ip, ix, d, rhs, np.zeros(n), 60, 1e-10, precond_diag=dg)          # checker: 28 iterations (25 with Jacobi)
    assert o.status == ref.OK and o.its == (28 if pc == "none" else 25)
    A = sa.HipCsr.new((n, n), ip, ix, d)
    s = sa.CG.new(A, n)
    x = np.zeros(n)
    st, its, res = _run(sa, s, P, rhs, x, 60, 1e-10)
    print("cfg3 %s: its %d (checker %d) res %.3e true %.3e kernel %s" % (pc, its, o.its, res, _true_res(ip, ix, d, rhs, x), A.spmv_route()["kernel"]))
    assert st == ref.OK and abs(its - o.its) <= _margin(o.its) and res <= 1e-10
    assert _true_res(ip, ix, d, rhs, x) <= 1e-9
    assert np.max(np.abs(x - o.x)) <= 1e-7 * np.max(np.abs(o.x))


def test_cfg5_operator_through_the_chains(sa):
    from test_gpu_dict_stream import _chain_cases
    ctx = sa.default_ctx(0)
    ip, ix, d, rhs = _chain_cases()["p3_160x128x24"]()[:4]
    n = rhs.size
    o = ref.cg(ip, ix, d, rhs, np.zeros(n), 600, 1e-10)                           # checker: 274 iterations
    assert o.status == ref.OK and 2 * o.its <= 600
    try:
        ctx.set("spmv_chain", 1); ctx.set("spmv_tile", 1)
        A = sa.HipCsr.new((n, n), ip, ix, d)
        assert A.chain_plan()[0] >= 64 and A.spmv_route()["kernel"] == "Chain", (A.chain_plan(), A.spmv_route())
        s = sa.CG.new(A, n)
        x = np.zeros(n)
        st, its, res = _run(sa, s, None, rhs, x, 600, 1e-10)
    finally:
        ctx.set("spmv_chain", -1); ctx.set("spmv_tile", -1)
    print("cfg5 operator: its %d (checker %d) res %.3e true %.3e" % (its, o.its, res, _true_res(ip, ix, d, rhs, x)))
    assert st == ref.OK and abs(its - o.its) <= _margin(o.its) and res <= 1e-10
    assert _true_res(ip, ix, d, rhs, x) <= 1e-9
