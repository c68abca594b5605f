"""ILU(0) on the GPU (sprs_ilu0_*, csrc/ilu0.hip) against the loops of tests/_ilu_ref.py: the factors and the triangular solves
BIT FOR BIT in all four scalar types (batched launches, per-level launches, partial slices, ragged rows, a level count above the
per-launch cap), the creation errors, and CG / GMRES preconditioned by it — literal mode against the checker and fused mode
against literal mode, with the comparisons and tolerances of tests/test_gpu_cg.py and tests/test_gpu_gmres.py (GMRES' trace rows over
the prefix that tests/test_ilu_cpu.py derives by test_gmres_cpu.py's rule: GMRES_TRACE_ROWS).

The checker's counts (tests/test_ilu_cpu.py: CG_COUNTS, GMRES_COUNTS) stand behind every max_iter, each at least twice its count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ilu_ref as ref  # noqa: E402
from test_gmres_cpu import trace_close as gm_trace_close  # noqa: E402
from test_ilu_cpu import ALL, C32, C64, CG_COUNTS, F32, F64, GMRES_COUNTS, GMRES_RESTART, GMRES_TRACE_ROWS, bits, factors_of, is_single, tol_of  # noqa: E402

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
    ip, ix, d, rhs, f = factors_of(name, np.dtype(dt).name)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    return ip, ix, d, rhs, f, A, sa.ILU0.new(A)


# ------------------------------------------------------------------------------------------------ 1. factors
@pytest.mark.parametrize("name,dt", [("cd24x20", F64), ("cd24x20", F32), ("herm300", C64), ("herm300", C32)], ids=_ids)
def test_factors_every_launch_a_batch(sa, name, dt):
    ip, ix, d, rhs, f, A, P = _handles(sa, name, dt)
    lv = P.levels
    want = ref.level_counts(ip, ix)
    print("%s %s: %s" % (name, np.dtype(dt).name, lv))
    assert (lv["lower_levels"], lv["upper_levels"]) == want
    assert np.bincount(ref.levels(ip, ix)[0]).max() <= 256                       # every level fits one workgroup ...
    assert lv["lower_launches"] == -(-want[0] // 128) and lv["upper_launches"] == -(-want[1] // 128)   # ... so every launch is a batch
    assert np.array_equal(bits(P.factors()), bits(f))
    A.close()                                                                     # the handle borrows nothing from A
    assert np.array_equal(bits(P.factors()), bits(f))


def test_factors_batched_and_per_level_launches(sa):
    ip, ix, d, rhs, f, A, P = _handles(sa, "p3_64x64x8", F64)
    lv = P.levels
    print("p3_64x64x8:", lv)
    assert lv["lower_levels"] == 134 and lv["upper_levels"] == 134
    assert 1 < lv["lower_launches"] < lv["lower_levels"] and 1 < lv["upper_launches"] < lv["upper_levels"]
    assert np.array_equal(bits(P.factors()), bits(f))


# ------------------------------------------------------------------------------------------------ 2. solves
SOLVE_CASES = [("cd24x20", F64), ("cd24x20", F32), ("herm300", C64), ("herm300", C32), ("p3_64x64x8", F64), ("tri300", F64), ("tri300", C32),
               ("ragged1000", F64), ("ragged1000", F32), ("ragged1000", C64)]


@pytest.mark.parametrize("name,dt", SOLVE_CASES, ids=_ids)
def test_solves_have_the_bits_of_the_serial_folds(sa, name, dt):
    ip, ix, d, rhs, f, A, P = _handles(sa, name, dt)
    n = rhs.size
    assert np.array_equal(bits(P.factors()), bits(f))
    ap = ref.Applier(ip, ix, f)
    lv = P.levels
    if name == "tri300":
        assert lv["lower_levels"] == 300 and lv["lower_launches"] == 3 and lv["upper_launches"] == 3       # 300 levels, 128 a launch
    apply = {0: P.mul_vec, 1: P.solve_lower, 2: P.solve_upper}
    for which in (1, 2, 0):
        want = ap.solve(which, rhs)
        out = np.zeros(n, dt)
        apply[which](rhs, out)                                                   # host entry point
        assert np.array_equal(bits(out), bits(want)), (which, "host")
        d_in = sa.DevVec.from_numpy(rhs); d_out = sa.DevVec.from_numpy(np.zeros(n, dt))
        apply[which](d_in, d_out)                                                # device entry point
        assert np.array_equal(bits(d_out.to_numpy()), bits(want)), (which, "device")
        apply[which](d_in, d_in)                                                 # in == out
        assert np.array_equal(bits(d_in.to_numpy()), bits(want)), (which, "in place")
    assert np.all(np.isfinite(ap.solve(0, rhs).view(np.float32 if is_single(dt) else np.float64)))


def test_solve_argument_checks(sa):
    from sprsolve_amd import _lib
    ip, ix, d, rhs, f, A, P = _handles(sa, "tri300", F64)
    n = rhs.size
    L = _lib.lib()
    out = np.zeros(n + 1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.sprs_ilu0_solve_d(P.h, 0, p(rhs.copy()), n - 1, p(out), n) == _lib.DIM_MISMATCH
    assert L.sprs_ilu0_solve_d(P.h, 0, p(rhs.copy()), n, p(out), n + 1) == _lib.DIM_MISMATCH
    assert L.sprs_ilu0_solve_d(P.h, 3, p(rhs.copy()), n, p(out), n) == _lib.INVALID_ARGUMENT
    assert L.sprs_ilu0_solve_d(P.h, -1, p(rhs.copy()), n, p(out), n) == _lib.INVALID_ARGUMENT
    assert L.sprs_ilu0_solve_s(P.h, 0, p(rhs.copy()), n, p(out), n) == _lib.INVALID_ARGUMENT      # another scalar type
    d_in = sa.DevVec.from_numpy(rhs)
    ptr = sa.device.dev_ptr(d_in)
    assert L.sprs_ilu0_solve_dev_d(P.h, 3, ptr, ptr) == _lib.INVALID_ARGUMENT
    assert L.sprs_ilu0_solve_dev_d(None, 0, ptr, ptr) == _lib.INVALID_ARGUMENT
    with pytest.raises(sa.error.DimensionMismatch):
        P.mul_vec(rhs[:-1], np.zeros(n - 1))
    assert L.sprs_ilu0_destroy(None) == 0
    assert not np.any(out)


# ------------------------------------------------------------------------------------------------ 3. creation errors
def test_creation_errors(sa):
    from sprsolve_amd import _lib
    E = sa.error
    ip = np.array([0, 2, 4], np.int32); ix = np.array([0, 1, 0, 1], np.int32)
    for dt in ALL:
        A = sa.HipCsr.new((2, 2), ip, ix, np.ones(4, dt))
        h = C.c_void_p(1); row = C.c_int64(-7)
        assert _lib.lib().sprs_ilu0_create(A.h, C.byref(h), C.byref(row)) == _lib.ZERO_DIAGONAL
        assert row.value == 1 and not h.value                                     # no handle
        with pytest.raises(E.ZeorDiagonalElem) as ei:
            sa.ILU0.new(A)
        assert ei.value.row == 1
    ip3 = np.array([0, 2, 3, 5, 6], np.int32); ix3 = np.array([0, 1, 0, 1, 2, 2], np.int32)
    with pytest.raises(E.ZeorDiagonalElem) as ei:                                 # rows 1 and 3 store no diagonal
        sa.ILU0.new(sa.HipCsr.new((4, 4), ip3, ix3, np.ones(6)))
    assert ei.value.row == 1
    with pytest.raises(E.ZeorDiagonalElem) as ei:                                 # a non-finite pivot
        sa.ILU0.new(sa.HipCsr.new((2, 2), ip, ix, np.array([np.inf, 1.0, 1.0, 1.0])))
    assert ei.value.row == 0
    for bad in (np.array([1, 0, 0, 1], np.int32), np.array([0, 1, 1, 1], np.int32)):   # unsorted; duplicate
        A = sa.HipCsr.new((2, 2), ip, bad, np.ones(4))
        h = C.c_void_p(1)
        assert _lib.lib().sprs_ilu0_create(A.h, C.byref(h), None) == _lib.INVALID_ARGUMENT and not h.value
        with pytest.raises(ValueError, match="strictly ascending"):
            sa.ILU0.new(A)
    with pytest.raises(E.IncompatibleMatrixFormat, match="Not a square"):
        sa.ILU0.new(sa.HipCsr.new((2, 3), ip, ix, np.ones(4)))
    # a handle created from CSC arrays is CSR by then
    from sprsolve_amd import gen
    tp, tx, td, _ = gen.random_tridiagonal(50)
    P = sa.ILU0.new(sa.HipCsr.new((50, 50), tp, tx, td, storage="CSC"))
    import scipy.sparse as sp
    At = sp.csc_matrix((td, tx, tp), shape=(50, 50)).tocsr(); At.sort_indices()
    assert np.array_equal(bits(P.factors()), bits(ref.ilu0(At.indptr, At.indices, At.data).val))


def test_distributed_operator_is_refused(sa):
    import torch
    from sprsolve_amd import dist as sdist, gen
    from test_gpu_dist import _self_halo_plan
    ctx = sa.default_ctx(0)
    dev = torch.device("cuda", 0)
    comm = sdist.Comm(ctx, 0, 1)
    try:
        n = 96 * 96
        ip, ix, d, rhs = gen.symmetric_banded(n)
        plan = _self_halo_plan(torch, dev, n, ix, lambda c: np.zeros(c.shape, bool))
        A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip).to(dev), torch.from_numpy(d).to(dev), adopt=True,
                                    to_device=lambda a: torch.from_numpy(a).to(dev))
        with pytest.raises(ValueError, match="distributed"):
            sa.ILU0.new(A)
        # ... and a single-GPU handle is refused by a solver on the distributed operator
        P = sa.ILU0.new(sa.HipCsr.new((n, n), ip, ix, d))
        with pytest.raises(ValueError):
            sa.CG.new(A, n).precond_solve(P, torch.from_numpy(rhs).to(dev), torch.zeros(n, dtype=torch.float64, device=dev), 10, 1e-10)
    finally:
        comm.close()


# ------------------------------------------------------------------------------------------------ 4. CG + ILU(0)
def _run(sa, solver, P, rhs, x, max_iter, tol):
    """-> (status, its, res) with the checker's status codes; x is updated in place."""
    E = sa.error
    try:
        its, res = solver.precond_solve(P, rhs, x, max_iter, tol)
        return ref.OK, its, res
    except E.InsufficientIterNum as e:
        return ref.INSUFFICIENT_ITER, e.iters, None
    except E.BreakDown as e:
        return ref.BREAKDOWN, e.its, None
    except E.InvalidPreconditioner as e:
        return ref.INVALID_PRECOND, None, e.msg


def _true_res(ip, ix, d, rhs, x):
    wide = np.complex128 if rhs.dtype.kind == "c" else np.float64
    A = ref._matvec(ip, ix, d.astype(wide))
    return np.linalg.norm(rhs.astype(wide) - A(x.astype(wide))) / np.linalg.norm(rhs.astype(wide))


def _cg_trace_close(a, b, rtol, atol=1e-8):
    """tests/test_gpu_cg.py's _trace_close."""
    def cx(t):
        t = np.atleast_2d(t)
        return np.concatenate([t[:, :2].astype(complex), t[:, 2::2] + 1j * t[:, 3::2]], axis=1)
    return np.allclose(cx(a), cx(b), rtol=rtol, atol=atol)


def _cg_trace_array(trace):
    return np.array([[t[0], t[1], t[2].real, t[2].imag, t[3].real, t[3].imag, t[4].real, t[4].imag] for t in trace]).reshape(-1, 8)


def _margin(its):
    return max(5, its // 4)                                  # tests/test_gpu_cg.py's


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_cg_literal_follows_the_checker_and_fused_follows_literal(sa, dt):
    ip, ix, d, rhs, f, A, P = _handles(sa, "cg", dt)
    n = rhs.size
    tol = tol_of(dt)
    max_iter = 2 * CG_COUNTS[np.dtype(dt).name][1]
    o = ref.cg(ip, ix, d, rhs, np.zeros(n, dt), max_iter, tol, prec=ref.Applier(ip, ix, f))
    assert o.status == ref.OK and 2 * o.its <= max_iter
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
    print("cg+ilu %s: literal its %d (checker %d) res %.3e (checker %.3e) max|x - checker| %.3e; fused its %d res %.3e true %.3e max|dx| %.3e"
          % (np.dtype(dt).name, il, o.its, rl, o.res, err, itf, rf, true_res, np.max(np.abs(xf - xl))))
    # literal against the checker (test_gpu_cg.py::test_literal_follows_the_checker)
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
    # fused against literal (test_gpu_cg.py::test_fused_follows_literal)
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert true_res <= 10 * tol
    if is_single(dt):
        assert np.max(np.abs(xf - xl)) < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert _cg_trace_close(tf[0], tl[0], rtol=1e-5)
    else:
        assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
        k = min(tf.shape[0], tl.shape[0])
        assert k >= il - 2 and _cg_trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)
    # without a trace buffer (lazy polling) and on device vectors the fused solve returns the same bits
    s = sa.CG.new(A, n)
    x2 = np.zeros(n, dt)
    assert _run(sa, s, P, rhs, x2, max_iter, tol)[:2] == (sf, itf) and np.array_equal(x2, xf)
    d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
    assert _run(sa, s, P, d_rhs, d_x, max_iter, tol)[:2] == (sf, itf) and np.array_equal(d_x.to_numpy(), xf)
    # the Jacobi path beside it is untouched, and needs more iterations
    rows = np.repeat(np.arange(n), np.diff(ip))
    J = sa.DiagPrecond.new(d[rows == ix].real.astype(np.float32 if is_single(dt) else np.float64).copy(), t_dtype=d.dtype)
    xj = np.zeros(n, dt)
    stj, itj, _ = _run(sa, s, J, rhs, xj, 2 * CG_COUNTS[np.dtype(dt).name][0], tol)
    assert stj == ref.OK and itj > itf


def test_cg_invalid_preconditioner_event(sa):
    ip, ix, d, rhs, f, A, P = _handles(sa, "indefinite", F64)
    n = rhs.size
    o = ref.cg(ip, ix, d, rhs, np.zeros(n), 50, 1e-10, prec=ref.Applier(ip, ix, f))
    assert (o.status, o.its) == (ref.INVALID_PRECOND, 3)
    for mode in ("fused", "literal"):
        s = sa.CG.new(A, n); s.set_mode(mode)
        x = np.zeros(n)
        with pytest.raises(sa.error.InvalidPreconditioner, match=r"beta_3 \[-0\.0018") as ei:
            s.precond_solve(P, rhs, x, 50, 1e-10)
        assert np.allclose(x, o.x, rtol=1e-9, atol=1e-12), (mode, ei.value)


# ------------------------------------------------------------------------------------------------ 5. GMRES + ILU(0)
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_gmres_literal_follows_the_checker_and_fused_follows_literal(sa, dt):
    ip, ix, d, rhs, f, A, P = _handles(sa, "cd24x20", dt)
    n = rhs.size
    tol = tol_of(dt)
    m = GMRES_RESTART
    max_iter = 2 * GMRES_COUNTS[np.dtype(dt).name][1]
    o = ref.gmres(ip, ix, d, rhs, np.zeros(n, dt), max_iter, tol, restart=m, prec=ref.Applier(ip, ix, f))
    assert o.status == ref.OK and 2 * o.its <= max_iter and o.its > m            # at least two cycles
    out = {}
    for mode in ("literal", "fused"):
        s = sa.GMRES.new(A, n, m); s.set_mode(mode); s.set_trace(max_iter)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace(), _true_res(ip, ix, d, rhs, x))
    (sl, il, rl, xl, tl, true_l), (sf, itf, rf, xf, tf, true_f) = out["literal"], out["fused"]
    want = np.array([[t[0], t[1], t[2], t[3].real, t[3].imag, t[4], t[5].real, t[5].imag] for t in o.trace]).reshape(-1, 8)
    err = np.max(np.abs(xl - o.x))
    print("gmres+ilu %s: literal its %d (checker %d) res %.3e (checker %.3e) true %.3e max|x - checker| %.3e; fused its %d res %.3e true %.3e max|dx| %.3e"
          % (np.dtype(dt).name, il, o.its, rl, o.res, true_l, err, itf, rf, true_f, np.max(np.abs(xf - xl))))
    # literal against the checker (test_gpu_gmres.py::test_literal_follows_the_checker)
    assert sl == o.status == ref.OK
    assert abs(il - o.its) <= _margin(o.its)
    assert tl.shape == (il, 8) and np.array_equal(tl[:, 0], np.arange(1, il + 1))
    assert rl <= tol and true_l <= 10 * tol
    k = min(GMRES_TRACE_ROWS, il, o.its)
    if is_single(dt):
        assert gm_trace_close(tl[:1], want[:1], rtol=1e-5, atol=1e-8)
        assert err < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
    else:
        assert gm_trace_close(tl[:k], want[:k], rtol=1e-9, atol=1e-12)
        assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
        assert il == o.its and np.isclose(rl, o.res, rtol=1e-9, atol=1e-12)
    # fused against literal (test_gpu_gmres.py::test_fused_follows_literal)
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert rf <= tol and true_f <= 10 * tol
    assert tf.shape == (itf, 8) and np.array_equal(tf[:, 0], np.arange(1, itf + 1))
    k = min(GMRES_TRACE_ROWS, itf, il)
    if is_single(dt):
        assert np.max(np.abs(xf - xl)) < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        assert gm_trace_close(tf[:1], tl[:1], rtol=1e-5, atol=1e-8)
    else:
        assert np.max(np.abs(xf - xl)) <= 1e-7 * np.max(np.abs(xl))
        assert gm_trace_close(tf[:k], tl[:k], rtol=1e-9, atol=1e-12)
        assert itf == il and np.isclose(rf, rl, rtol=1e-9, atol=1e-12)
    # lazy polling and device vectors: the same bits
    s = sa.GMRES.new(A, n, m)
    x2 = np.zeros(n, dt)
    assert _run(sa, s, P, rhs, x2, max_iter, tol)[:2] == (sf, itf) and np.array_equal(x2, xf)
    d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
    assert _run(sa, s, P, d_rhs, d_x, max_iter, tol)[:2] == (sf, itf) and np.array_equal(d_x.to_numpy(), xf)


# ------------------------------------------------------------------------------------------------ 6. the wrong handle
def test_wrong_handle_is_refused_by_the_solvers(sa):
    from sprsolve_amd import _lib
    ip, ix, d, rhs, f, A, P = _handles(sa, "cd24x20", F64)
    n = rhs.size
    _, _, _, _, _, A32, P32 = _handles(sa, "cd24x20", F32)
    _, _, _, _, _, _, Psmall = _handles(sa, "tri300", F64)
    for mk in (lambda: sa.CG.new(A, n), lambda: sa.GMRES.new(A, n, 5)):
        x = np.zeros(n)
        with pytest.raises(ValueError):
            mk().precond_solve(P32, rhs, x, 10, 1e-10)                            # another scalar type
        with pytest.raises(sa.error.DimensionMismatch):
            mk().precond_solve(Psmall, rhs, x, 10, 1e-10)                         # another size
        assert not np.any(x)
    its = C.c_size_t(); res = C.c_double(); x = np.zeros(n)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for name, s in (("cg", sa.CG.new(A, n)), ("gmres", sa.GMRES.new(A, n, 5))):
        fn = getattr(_lib.lib(), "sprs_ilu0_%s_solve_d" % name)
        assert fn(s.h, None, p(rhs.copy()), n, p(x), n, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INVALID_ARGUMENT
        assert fn(s.h, P.h, p(rhs.copy()), n - 1, p(x), n, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INCOMPATIBLE_RHS_SIZE
        assert fn(s.h, P.h, p(rhs.copy()), n, p(x), n + 1, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INCOMPATIBLE_X_SIZE
