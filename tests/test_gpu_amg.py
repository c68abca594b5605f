"""Smoothed-aggregation AMG on the GPU (sprs_amg_*, csrc/amg.hip) against tests/_amg_ref.py: the hierarchy read back level by
level (aggregates and patterns exact, values BIT FOR BIT in all four scalar types: the complex host arithmetic is the naive
component formulas compiled without contraction, so it is pinned like the real one), one application of the cycle bit for bit
(multi-workgroup levels, a partial last slice, the tail kernel taking over mid-hierarchy, and hierarchies that fit the tail
entirely; in == out and in != out), the creation errors, and CG / GMRES preconditioned by it — literal mode against the checker
and fused mode against literal mode with the comparisons and tolerances of tests/test_gpu_ilu.py (GMRES' trace rows over
GMRES_TRACE_ROWS, the prefix tests/test_amg_cpu.py derives).

The checker's counts (tests/test_amg_cpu.py) stand behind every max_iter, each at least twice its count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _amg_ref as amg  # noqa: E402
import _ilu_ref as ref  # noqa: E402
from test_amg_cpu import (ALL, C32, C64, CG_COUNTS, CG_MAX_ITER, F32, F64, GMRES_COUNTS, GMRES_MAX_ITER, GMRES_RESTART,  # noqa: E402
                          GMRES_TRACE_ROWS, INDEFINITE, MAX_LEVELS, THETA, bits, hierarchy_of, system_of, tol_of)
from test_gmres_cpu import trace_close as gm_trace_close  # noqa: E402
from test_gpu_ilu import _cg_trace_array, _cg_trace_close, _margin, _run, _true_res  # noqa: E402
from test_ilu_cpu import is_single  # noqa: E402

pytestmark = pytest.mark.gpu

_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


def _handles(sa, name, dt):
    ip, ix, d, rhs = system_of(name, np.dtype(dt).name)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    return ip, ix, d, rhs, hierarchy_of(name, np.dtype(dt).name), A, sa.AMG.new(A)


# ------------------------------------------------------------------------------------------------ 1. the hierarchy
@pytest.mark.parametrize("name,dt", [("p3_12x11x10", F64), ("p3_12x11x10", C64), ("p3_24x22x20", F64), ("cd24x20", F64), ("cd24x20", F32), ("cd24x20", C32),
                                     ("tri300", F64), ("tri300", F32), ("ragged1000", F64), ("ragged1000", F32)], ids=_ids)
def test_hierarchy_equals_the_checkers(sa, name, dt):
    ip, ix, d, rhs, H, A, P = _handles(sa, name, dt)
    A.close()                                                                     # the handle borrows nothing from A
    inf = P.info
    print(name, np.dtype(dt).name, inf)
    assert inf["levels"] == len(H.levels) and inf["rows"] == [L.n for L in H.levels]
    assert inf["nnz"] == [int(L.ip[-1]) for L in H.levels]
    assert inf["lu_rows"] == (H.levels[-1].n if H.lu is not None else 0)
    for l, L in enumerate(H.levels):
        assert bits(np.array([inf["omega"][l]], amg.Ops(dt).R)).tolist() == bits(np.array([L.omega])).tolist()
        for which, want in (("A", (L.ip, L.ix, L.val)), ("P", L.P), ("R", L.R)):
            if want is None:
                continue
            gp, gx, gv = P.level(l, which)
            assert np.array_equal(gp, want[0]) and np.array_equal(gx, want[1]), (l, which)
            assert np.array_equal(bits(gv), bits(want[2])), (l, which)
        if L.agg is not None:
            assert np.array_equal(P.aggregates(l), L.agg), l
    last = len(H.levels) - 1                                                      # the coarsest level has no P, R or aggregates
    for bad in (lambda: P.level(last, "P"), lambda: P.level(last, "R"), lambda: P.aggregates(last), lambda: P.level(last + 1), lambda: P.level(-1)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ 2. one application
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_cycle_bits_with_multi_workgroup_levels_and_the_tail(sa, dt):
    """poisson3d(64, 64, 8): 32 768 and 4133 rows run the multi-workgroup kernels (4133 = 64 * 64 + 37: a partial last slice),
    two more levels the tail kernel, which ends in the dense LU.  The strength test rounds in the scalar type, so from level 2 on
    the sizes depend on it (f64: 445 and 34 rows, c64: 424 and 75); they are the checker's."""
    ip, ix, d, rhs, H, A, P = _handles(sa, "p3_64x64x8", dt)
    inf = P.info
    print(np.dtype(dt).name, inf)
    rows = [L.n for L in H.levels]
    assert rows[:2] == [32768, 4133] and len(rows) == 4 and 256 < rows[2] <= 1024 and H.lu is not None
    if np.dtype(dt) == np.dtype(F64):
        assert rows == [32768, 4133, 445, 34]
    assert inf["rows"] == rows and inf["tail_level"] == 2 and inf["lu_rows"] == rows[3]
    assert inf["launches"] == 5 * 2 + 1
    want = amg.Applier(H)(rhs)
    out = np.zeros_like(rhs)
    P.mul_vec(rhs, out)                                                           # host arrays, in != out
    assert np.array_equal(bits(out), bits(want))
    v = sa.DevVec.from_numpy(rhs)
    P.mul_vec(v, v)                                                               # device vectors, in == out
    assert np.array_equal(bits(v.to_numpy()), bits(want))
    a, b = sa.DevVec.from_numpy(rhs), sa.DevVec.from_numpy(np.zeros_like(rhs))
    P.mul_vec(a, b)
    assert np.array_equal(bits(b.to_numpy()), bits(want)) and np.array_equal(bits(a.to_numpy()), bits(rhs))


@pytest.mark.parametrize("name,dt", [("p3_8x7x6", F64), ("p3_8x7x6", C64), ("p3_8x7x6", F32), ("p3_8x7x6", C32), ("ragged1000", F64),
                                     ("cd24x20", C64)], ids=_ids)
def test_cycle_bits_inside_the_tail_kernel_alone(sa, name, dt):
    ip, ix, d, rhs, H, A, P = _handles(sa, name, dt)
    inf = P.info
    assert inf["tail_level"] == 0 and inf["launches"] == 1 and inf["levels"] == len(H.levels) >= 2
    want = amg.Applier(H)(rhs)
    out = np.zeros_like(rhs)
    P.mul_vec(rhs, out)
    assert np.array_equal(bits(out), bits(want))
    v = sa.DevVec.from_numpy(rhs)
    P.mul_vec(v, v)
    assert np.array_equal(bits(v.to_numpy()), bits(want))


@pytest.mark.parametrize("name,n_upper", [("tri300", 0), ("p3_12x11x10", 1)], ids=["tri300", "p3_12x11x10"])
def test_cycle_bits_with_jacobi_sweeps_for_the_coarse_solve(sa, name, n_upper):
    """theta = 10 leaves only singletons: the half-rows stop makes level 0 the coarsest, and eight Jacobi sweeps stand for the
    coarse solve — inside the tail kernel (300 rows) and as launches of their own (1320 rows, above the tail)."""
    ip, ix, d, rhs = system_of(name, "float64")
    n = rhs.size
    H = amg.build(ip, ix, d, 10.0, 16, MAX_LEVELS)
    P = sa.AMG.new(sa.HipCsr.new((n, n), ip, ix, d), theta=10.0, coarse_max=16)
    inf = P.info
    assert len(H.levels) == 1 and H.lu is None and inf["levels"] == 1 and inf["lu_rows"] == 0
    assert inf["tail_level"] == (0 if n_upper == 0 else 1) and inf["launches"] == (1 if n_upper == 0 else amg.COARSE_SWEEPS)
    want = amg.Applier(H)(rhs)
    for same in (False, True):
        a = sa.DevVec.from_numpy(rhs)
        b = a if same else sa.DevVec.from_numpy(np.zeros_like(rhs))
        P.mul_vec(a, b)
        assert np.array_equal(bits(b.to_numpy()), bits(want)), same


# ------------------------------------------------------------------------------------------------ 3. creation errors
def test_creation_errors(sa):
    E = sa.error
    ip = np.array([0, 2, 4], np.int32); ix = np.array([0, 1, 0, 1], np.int32)
    for dt in ALL:
        with pytest.raises(E.ZeorDiagonalElem) as ei:                             # the coarse LU: u_11 = 1 - 1*1
            sa.AMG.new(sa.HipCsr.new((2, 2), ip, ix, np.ones(4, dt)))
        assert "1" in str(ei.value)
    ip3 = np.array([0, 2, 3, 5, 6], np.int32); ix3 = np.array([0, 1, 0, 1, 2, 2], np.int32)
    with pytest.raises(E.ZeorDiagonalElem) as ei:                                 # a missing diagonal
        sa.AMG.new(sa.HipCsr.new((4, 4), ip3, ix3, np.ones(6)))
    assert "1" in str(ei.value)
    with pytest.raises(E.ZeorDiagonalElem):                                       # a zero diagonal
        sa.AMG.new(sa.HipCsr.new((2, 2), ip, ix, np.array([1.0, 1.0, 1.0, 0.0])))
    with pytest.raises(E.IncompatibleMatrixFormat):
        sa.AMG.new(sa.HipCsr.new((2, 3), ip, np.array([0, 2, 0, 1], np.int32), np.ones(4)))
    A = sa.HipCsr.new((2, 2), ip, ix, np.array([2.0, 1.0, 1.0, 2.0]))
    for kw in (dict(theta=-1.0), dict(coarse_max=0), dict(coarse_max=amg.COARSE_LIMIT + 1), dict(max_levels=0),
               dict(max_levels=amg.LEVELS_LIMIT + 1)):
        with pytest.raises(ValueError):
            sa.AMG.new(A, **kw)
    P = sa.AMG.new(A)
    with pytest.raises(sa.error.DimensionMismatch):
        P.mul_vec(np.ones(3), np.zeros(3))


# ------------------------------------------------------------------------------------------------ 4. CG + AMG
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_cg_literal_follows_the_checker_and_fused_follows_literal(sa, dt):
    ip, ix, d, rhs, H, A, P = _handles(sa, "cg", dt)
    n = rhs.size
    tol = tol_of(dt)
    max_iter = CG_MAX_ITER
    o = ref.cg(ip, ix, d, rhs, np.zeros(n, dt), max_iter, tol, prec=amg.Applier(H))
    assert o.status == ref.OK and o.its == CG_COUNTS[np.dtype(dt).name][1] and 2 * o.its <= max_iter
    out = {}
    for mode in ("literal", "fused"):
        s = sa.CG.new(A, n); s.set_mode(mode); s.set_trace(max_iter)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace())
    (sl, il, rl, xl, tl), (sf, itf, rf, xf, tf) = out["literal"], out["fused"]
    want = _cg_trace_array(o.trace)
    err = np.max(np.abs(xl - o.x))
    true_res = _true_res(ip, ix, d, rhs, xf)
    print("cg+amg %s: literal its %d (checker %d) res %.3e (checker %.3e) max|x - checker| %.3e; fused its %d res %.3e true %.3e max|dx| %.3e"
          % (np.dtype(dt).name, il, o.its, rl, o.res, err, itf, rf, true_res, np.max(np.abs(xf - xl))))
    # literal against the checker: status and iteration count equal
    assert (sl, il) == (o.status, o.its)
    assert tl.shape == want.shape == (o.its - 1, 8)
    if is_single(dt):
        assert _cg_trace_close(tl[0], want[0], rtol=1e-5)
        assert err < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert rl <= tol
    else:
        assert _cg_trace_close(tl, want, rtol=1e-9, atol=1e-12)
        assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
        assert np.isclose(rl, o.res, rtol=1e-9, atol=1e-12)
    # fused against literal
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert true_res <= 10 * tol
    if is_single(dt):
        assert np.max(np.abs(xf - xl)) < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert _cg_trace_close(tf[0], tl[0], rtol=1e-5)
    else:
        assert itf == il
        assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
        k = min(tf.shape[0], tl.shape[0])
        assert k >= il - 2 and _cg_trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)
    # without a trace buffer (lazy polling) and on device vectors the fused solve returns the same bits
    s = sa.CG.new(A, n)
    x2 = np.zeros(n, dt)
    assert _run(sa, s, P, rhs, x2, max_iter, tol)[:2] == (sf, itf) and np.array_equal(x2, xf)
    d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
    assert _run(sa, s, P, d_rhs, d_x, max_iter, tol)[:2] == (sf, itf) and np.array_equal(d_x.to_numpy(), xf)


def test_cg_invalid_preconditioner_event(sa):
    ip, ix, d, rhs, H, A, P = _handles(sa, "indefinite", F64)
    n = rhs.size
    o = ref.cg(ip, ix, d, rhs, np.zeros(n), CG_MAX_ITER, 1e-10, prec=amg.Applier(H))
    assert (o.status, o.its) == (ref.INVALID_PRECOND, INDEFINITE[0])
    for mode in ("fused", "literal"):
        s = sa.CG.new(A, n); s.set_mode(mode)
        x = np.zeros(n)
        with pytest.raises(sa.error.InvalidPreconditioner, match=r"beta_%d \[-2\.3" % INDEFINITE[0]) as ei:
            s.precond_solve(P, rhs, x, CG_MAX_ITER, 1e-10)
        assert np.allclose(x, o.x, rtol=1e-9, atol=1e-12), (mode, ei.value)


# ------------------------------------------------------------------------------------------------ 5. GMRES + AMG
@pytest.mark.parametrize("dt", [F64, C64], ids=_ids)
def test_gmres_literal_follows_the_checker_and_fused_follows_literal(sa, dt):
    ip, ix, d, rhs, H, A, P = _handles(sa, "cd24x20", dt)
    n = rhs.size
    tol = 1e-10
    m = GMRES_RESTART
    max_iter = GMRES_MAX_ITER
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), max_iter, tol, restart=m, prec=amg.Applier(H))
    assert o.status == ref.OK and o.its == GMRES_COUNTS[np.dtype(dt).name][1] and 2 * o.its <= max_iter and o.its > m
    out = {}
    for mode in ("literal", "fused"):
        s = sa.GMRES.new(A, n, m); s.set_mode(mode); s.set_trace(max_iter)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace(), _true_res(ip, ix, d, rhs, x))
    (sl, il, rl, xl, tl, true_l), (sf, itf, rf, xf, tf, true_f) = out["literal"], out["fused"]
    want = np.array([[t[0], t[1], t[2], t[3].real, t[3].imag, t[4], t[5].real, t[5].imag] for t in o.trace]).reshape(-1, 8)
    err = np.max(np.abs(xl - o.x))
    print("gmres+amg %s: literal its %d (checker %d) res %.3e (checker %.3e) true %.3e max|x - checker| %.3e; fused its %d res %.3e true %.3e max|dx| %.3e"
          % (np.dtype(dt).name, il, o.its, rl, o.res, true_l, err, itf, rf, true_f, np.max(np.abs(xf - xl))))
    assert sl == o.status == ref.OK and il == o.its
    assert tl.shape == (il, 8) and np.array_equal(tl[:, 0], np.arange(1, il + 1))
    assert rl <= tol and true_l <= 10 * tol
    k = GMRES_TRACE_ROWS
    assert gm_trace_close(tl[:k], want[:k], rtol=1e-9, atol=1e-12)
    assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
    assert np.isclose(rl, o.res, rtol=1e-9, atol=1e-12)
    assert sf == sl and itf == il
    assert rf <= tol and true_f <= 10 * tol
    assert tf.shape == (itf, 8) and np.array_equal(tf[:, 0], np.arange(1, itf + 1))
    assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
    assert gm_trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)
    assert np.isclose(rf, rl, rtol=1e-9, atol=1e-12)
    d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
    s = sa.GMRES.new(A, n, m)
    assert _run(sa, s, P, d_rhs, d_x, max_iter, tol)[:2] == (sf, itf) and np.array_equal(d_x.to_numpy(), xf)


# ------------------------------------------------------------------------------------------------ 6. the wrong handle
def test_wrong_handle_is_refused_by_the_solvers(sa):
    from sprsolve_amd import _lib
    ip, ix, d, rhs, H, A, P = _handles(sa, "cd24x20", F64)
    n = rhs.size
    _, _, _, _, _, _, P32 = _handles(sa, "cd24x20", F32)
    _, _, _, _, _, _, Psmall = _handles(sa, "tri300", F64)
    ctx2 = sa.Context(0)
    Pother = sa.AMG.new(sa.HipCsr.new((n, n), ip, ix, d, ctx=ctx2))
    for mk in (lambda: sa.CG.new(A, n), lambda: sa.GMRES.new(A, n, 5)):
        x = np.zeros(n)
        with pytest.raises(ValueError):
            mk().precond_solve(P32, rhs, x, 10, 1e-10)                            # another scalar type
        with pytest.raises(ValueError):
            mk().precond_solve(Pother, rhs, x, 10, 1e-10)                         # another context
        with pytest.raises(sa.error.DimensionMismatch):
            mk().precond_solve(Psmall, rhs, x, 10, 1e-10)                         # another size
        assert not np.any(x)
    its = C.c_size_t(); res = C.c_double(); x = np.zeros(n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for name, s in (("cg", sa.CG.new(A, n)), ("gmres", sa.GMRES.new(A, n, 5))):
        fn = getattr(_lib.lib(), "sprs_amg_%s_solve_d" % name)
        assert fn(s.h, None, p(rhs.copy()), n, p(x), n, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INVALID_ARGUMENT
        assert fn(s.h, P.h, p(rhs.copy()), n - 1, p(x), n, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INCOMPATIBLE_RHS_SIZE
