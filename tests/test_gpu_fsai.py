"""FSAI on the GPU (sprs_fsai_*, csrc/fsai.hip) against the loops of tests/_fsai_ref.py: the pattern and the values of G BIT FOR BIT
in all four scalar types and both powers (every length bin, many workgroups, a partial last group, mixed row lengths inside one
group), the row cap, the application against the two row folds, the creation errors, and CG, MINRES, BiCGStab and GMRES
preconditioned by it — literal mode against the project's checkers fed with the checker's apply, fused mode against literal mode,
with the comparisons and tolerances of tests/test_gpu_ilu.py and tests/test_gpu_krylov_prec.py (imported, none invented).

The checkers' counts (tests/test_fsai_cpu.py: FSAI_CG_COUNTS, FSAI_KRYLOV_COUNTS) stand behind every max_iter, each at least twice
its count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _fsai_ref as fr  # noqa: E402
import _ilu_ref as ref  # noqa: E402
import _krylov_prec_ref as kp  # noqa: E402
from test_fsai_cpu import (ALL, C32, C64, F32, F64, FSAI_CG_COUNTS, GMRES_RESTART, POWERS, SYSTEMS, applier, bits, checker_run, dense_hpd, factor_of,  # noqa: E402,F401
                           gmres_trace_array, is_single, max_iter_of, system, tol_of, trace_prefix)
from test_gmres_cpu import trace_close as gm_trace_close  # noqa: E402
from test_gpu_ilu import _cg_trace_array, _cg_trace_close, _margin, _run, _true_res  # noqa: E402
from test_krylov_prec_cpu import gpu_tols  # noqa: E402

pytestmark = pytest.mark.gpu

_ids = lambda v: v if isinstance(v, str) else (np.dtype(v).name if isinstance(v, type) else str(v))


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


def _handles(sa, name, dt, power=1):
    ip, ix, d, rhs = dense_hpd(int(name[5:]), np.dtype(dt).name) if name.startswith("dense") else system(name, np.dtype(dt).name)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    return ip, ix, d, rhs, A, sa.FSAI.new(A, power=power)


def _same_factor(P, f):
    gp, gx, gv = P.factor()
    assert np.array_equal(gp, f.ip) and np.array_equal(gx, f.ix), "pattern"
    assert gv.dtype == f.val.dtype and np.array_equal(bits(gv), bits(f.val)), "values"
    inf = P.info
    assert (inf["n"], inf["nnz"], inf["max_row"]) == (f.ip.size - 1, f.ix.size, int(np.diff(f.ip).max()))


# ------------------------------------------------------------------------------------------------ 1. factor bits
@pytest.mark.parametrize("power", POWERS)
@pytest.mark.parametrize("dt", ALL, ids=_ids)
@pytest.mark.parametrize("name", SYSTEMS)
def test_factor_has_the_bits_of_the_checker(sa, name, dt, power):
    ip, ix, d, rhs, A, P = _handles(sa, name, dt, power)
    f = factor_of(name, np.dtype(dt).name, power)
    assert P.info["power"] == power
    _same_factor(P, f)


def test_factor_over_many_workgroups(sa):
    """poisson3d(64, 64, 8): 32 768 rows of 1 .. 4 entries — 1024 workgroups of the shortest bin — and nothing else."""
    ip, ix, d, rhs, A, P = _handles(sa, "p3_64x64x8", F64)
    f = factor_of("p3_64x64x8", "float64", 1)
    assert sorted(set(np.diff(f.ip))) == [1, 2, 3, 4]
    _same_factor(P, f)


# ------------------------------------------------------------------------------------------------ 2. mixed row lengths
@pytest.mark.parametrize("dt", [F64, C64], ids=_ids)
def test_dense_matrix_mixes_row_lengths_in_one_group_and_inverts(sa, dt):
    """The dense 24 x 24 matrix: rows of 1 .. 24 entries, so the bins <= 8, <= 16 and <= 32 each hold rows of different lengths in
    one workgroup.  G^H G = A^-1 there: mul_vec of A v returns v."""
    ip, ix, d, rhs, A, P = _handles(sa, "dense24", dt)
    f = factor_of("dense24", np.dtype(dt).name, 1)
    assert np.array_equal(np.diff(f.ip), np.arange(1, 25))
    _same_factor(P, f)
    Av = fr.dense(ip, ix, d) @ rhs
    out = np.zeros(24, dt)
    P.mul_vec(Av, out)
    err = np.max(np.abs(out - rhs)) / np.max(np.abs(rhs))
    print("dense24 %s: |M A v - v| / |v| = %.2e" % (np.dtype(dt).name, err))
    assert err <= 1e-12


# ------------------------------------------------------------------------------------------------ 3. the cap
def test_row_cap(sa):
    from sprsolve_amd import _lib, gen
    ip, ix, d, rhs = dense_hpd(70, "float64")
    A = sa.HipCsr.new((70, 70), ip, ix, d)
    h = C.c_void_p(1); row = C.c_int64(-7)
    assert _lib.lib().sprs_fsai_create(A.h, 1, C.byref(h), C.byref(row)) == _lib.INVALID_ARGUMENT and not h.value and row.value == -1
    with pytest.raises(ValueError, match=r"row 64 of G has 65 entries"):
        sa.FSAI.new(A)
    # ... and a 64-entry row is allowed: the leading 64 x 64 block (the longest bin, one row a workgroup)
    keep = (np.repeat(np.arange(70), 70) < 64) & (ix < 64)
    ip64 = (np.arange(65) * 64).astype(np.int32)
    A64 = sa.HipCsr.new((64, 64), ip64, ix[keep], d[keep])
    P = sa.FSAI.new(A64)
    assert P.info["max_row"] == 64
    f = fr.fsai(ip64, ix[keep], d[keep], 1, rows=[0, 40, 63])
    gp, gx, gv = P.factor()
    assert np.array_equal(gp, f.ip) and np.array_equal(gx, f.ix)
    for i in (0, 40, 63):
        assert np.array_equal(bits(gv[gp[i]:gp[i + 1]]), bits(f.val[gp[i]:gp[i + 1]])), i
    # symmetric_banded(2000, hbw=8) squared: the longest row has 17 entries, the <= 32 bin
    bp, bx, bd, _ = gen.symmetric_banded(2000, hbw=8)
    P = sa.FSAI.new(sa.HipCsr.new((2000, 2000), bp, bx, bd), power=2)
    assert P.info["max_row"] == 17
    rows = [0, 7, 16, 1000, 1999]
    f = fr.fsai(bp, bx, bd, 2, rows=rows)
    gp, gx, gv = P.factor()
    assert np.array_equal(gp, f.ip) and np.array_equal(gx, f.ix)
    for i in rows:
        assert np.array_equal(bits(gv[gp[i]:gp[i + 1]]), bits(f.val[gp[i]:gp[i + 1]])), i


# ------------------------------------------------------------------------------------------------ 4. application
@pytest.mark.parametrize("power", POWERS)
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_application_has_the_bits_of_the_two_folds(sa, dt, power):
    ip, ix, d, rhs, A, P = _handles(sa, "cg", dt, power)
    n = rhs.size
    want = applier("cg", np.dtype(dt).name, power)(rhs)
    out = np.zeros(n, dt)
    P.mul_vec(rhs, out)                                                          # host entry point
    assert np.array_equal(bits(out), bits(want)), "host"
    d_in = sa.DevVec.from_numpy(rhs); d_out = sa.DevVec.from_numpy(np.zeros(n, dt))
    P.mul_vec(d_in, d_out)                                                       # device entry point
    assert np.array_equal(bits(d_out.to_numpy()), bits(want)), "device"
    P.mul_vec(d_in, d_in)                                                        # in is out
    assert np.array_equal(bits(d_in.to_numpy()), bits(want)), "in place"
    A.close()                                                                    # the handle borrows nothing from A
    out2 = np.zeros(n, dt)
    P.mul_vec(rhs, out2)
    assert np.array_equal(bits(out2), bits(want)), "after A.close()"
    with pytest.raises(sa.error.DimensionMismatch):
        P.mul_vec(rhs[:-1], np.zeros(n - 1, dt))
    with pytest.raises(NotImplementedError):
        P.mul_vec_dot(rhs, out)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_creation_errors(sa):
    from sprsolve_amd import _lib
    E = sa.error
    ip, ix, d, rhs = system("indefinite", "float64")
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    for power in POWERS:
        h = C.c_void_p(1); row = C.c_int64(-7)
        assert _lib.lib().sprs_fsai_create(A.h, power, C.byref(h), C.byref(row)) == _lib.INVALID_PRECOND
        assert row.value == 15 and not h.value                                    # no handle
        with pytest.raises(E.InvalidPreconditioner, match="not positive definite on the pattern at row 15"):
            sa.FSAI.new(A, power=power)
    bp, bx, bd, _ = system("banded", "float64")
    rows = np.repeat(np.arange(bp.size - 1), np.diff(bp))
    for row in (0, 137, 299):
        keep = ~((rows == row) & (bx == row))
        ip2 = np.zeros_like(bp); np.cumsum(np.bincount(rows[keep], minlength=bp.size - 1), out=ip2[1:])
        for power in POWERS:
            with pytest.raises(E.ZeorDiagonalElem) as ei:
                sa.FSAI.new(sa.HipCsr.new((300, 300), ip2, bx[keep], bd[keep]), power=power)
            assert ei.value.row == row
    # a zero diagonal wins over a row that is not positive definite
    keep = ~((np.repeat(np.arange(n), np.diff(ip)) == 40) & (ix == 40))
    ip2 = np.zeros_like(ip); np.cumsum(np.bincount(np.repeat(np.arange(n), np.diff(ip))[keep], minlength=n), out=ip2[1:])
    with pytest.raises(E.ZeorDiagonalElem) as ei:
        sa.FSAI.new(sa.HipCsr.new((n, n), ip2, ix[keep], d[keep]))
    assert ei.value.row == 40
    ipb = np.array([0, 2, 4], np.int32); ixb = np.array([0, 1, 0, 1], np.int32)
    with pytest.raises(E.IncompatibleMatrixFormat, match="Not a square"):
        sa.FSAI.new(sa.HipCsr.new((2, 3), ipb, ixb, np.ones(4)))
    Ab = sa.HipCsr.new((2, 2), ipb, ixb, np.array([2.0, 1.0, 1.0, 2.0]))
    for power in (0, 3, -1):
        with pytest.raises(ValueError, match="power"):
            sa.FSAI.new(Ab, power=power)
        h = C.c_void_p(1)
        assert _lib.lib().sprs_fsai_create(Ab.h, power, C.byref(h), None) == _lib.INVALID_ARGUMENT and not h.value
    for bad in (np.array([1, 0, 0, 1], np.int32), np.array([0, 1, 1, 1], np.int32)):   # unsorted; duplicate
        with pytest.raises(ValueError, match="strictly ascending"):
            sa.FSAI.new(sa.HipCsr.new((2, 2), ipb, bad, np.ones(4)))
    assert _lib.lib().sprs_fsai_destroy(None) == 0
    # only the lower triangle is read: garbage above the diagonal changes nothing
    up = bd.copy(); up[bx > rows] = 1e30
    f = factor_of("banded", "float64", 1)
    _same_factor(sa.FSAI.new(sa.HipCsr.new((300, 300), bp, bx, up)), f)


def test_distributed_operator_is_refused(sa):
    """tests/test_gpu_ilu.py::test_distributed_operator_is_refused for FSAI."""
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
            sa.FSAI.new(A)
        # ... and a single-GPU handle is refused by a solver on the distributed operator
        P = sa.FSAI.new(sa.HipCsr.new((n, n), ip, ix, d))
        with pytest.raises(ValueError):
            sa.CG.new(A, n).precond_solve(P, torch.from_numpy(rhs).to(dev), torch.zeros(n, dtype=torch.float64, device=dev), 10, 1e-10)
    finally:
        comm.close()


def test_wrong_handle_is_refused_by_the_solvers(sa):
    """The statuses of applied_check, through CG.precond_solve and the three other solvers."""
    from sprsolve_amd import _lib
    ip, ix, d, rhs, A, P = _handles(sa, "cg", F64)
    n = rhs.size
    _, _, _, _, _, P32 = _handles(sa, "cg", F32)
    _, _, _, _, _, Psmall = _handles(sa, "banded", F64)
    ctx2 = sa.Context(0)
    Pother = sa.FSAI.new(sa.HipCsr.new((n, n), ip, ix, d, ctx=ctx2))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for sname, mk in (("cg", lambda: sa.CG.new(A, n)), ("gmres", lambda: sa.GMRES.new(A, n, 5)), ("bicgstab", lambda: sa.BiCGStab.new(A, n)),
                      ("minres", lambda: sa.MinRes.new(A, n))):
        x = np.zeros(n)
        with pytest.raises(ValueError):
            mk().precond_solve(P32, rhs, x, 10, 1e-10)                            # another scalar type
        with pytest.raises(ValueError):
            mk().precond_solve(Pother, rhs, x, 10, 1e-10)                         # another context
        with pytest.raises(sa.error.DimensionMismatch):
            mk().precond_solve(Psmall, rhs, x, 10, 1e-10)                         # another size
        assert not np.any(x)
        its = C.c_size_t(); res = C.c_double(); s = mk()
        fn = getattr(_lib.lib(), "sprs_fsai_%s_solve_d" % sname)
        assert fn(s.h, None, p(rhs.copy()), n, p(x), n, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INVALID_ARGUMENT
        assert fn(s.h, P.h, p(rhs.copy()), n - 1, p(x), n, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INCOMPATIBLE_RHS_SIZE
        assert fn(s.h, P.h, p(rhs.copy()), n, p(x), n + 1, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INCOMPATIBLE_X_SIZE
        assert not np.any(x)


# ------------------------------------------------------------------------------------------------ 6. solves
CG_CASES = [(name, dt, power) for name in SYSTEMS for dt in ALL for power in POWERS]


@pytest.mark.parametrize("name,dt,power", CG_CASES, ids=_ids)
def test_cg_literal_follows_the_checker_and_fused_follows_literal(sa, name, dt, power):
    """tests/test_gpu_ilu.py::test_cg_literal_follows_the_checker_and_fused_follows_literal with M = FSAI."""
    dtname = np.dtype(dt).name
    ip, ix, d, rhs, A, P = _handles(sa, name, dt, power)
    n = rhs.size
    tol = tol_of(dt)
    max_iter = max_iter_of("cg", name, dtname, power)
    o = checker_run("cg", name, dtname, power)
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
    print("cg+fsai(%d) %s %s: literal its %d (checker %d) res %.3e (checker %.3e) max|x - checker| %.3e; fused its %d res %.3e true %.3e max|dx| %.3e"
          % (power, name, dtname, il, o.its, rl, o.res, err, itf, rf, true_res, np.max(np.abs(xf - xl))))
    # literal against the checker
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
    stj, itj, _ = _run(sa, s, J, rhs, xj, 2 * FSAI_CG_COUNTS[name][dtname][0], tol)
    assert stj == ref.OK and itj > itf


KRYLOV_CASES = [(solver, name, dt) for solver in ("bicgstab", "minres") for name in SYSTEMS for dt in ALL]


@pytest.mark.parametrize("solver,name,dt", KRYLOV_CASES, ids=_ids)
def test_bicgstab_and_minres_follow_the_checker(sa, solver, name, dt):
    """tests/test_gpu_krylov_prec.py::_follows with M = FSAI(power 1)."""
    dtname = np.dtype(dt).name
    cls = {"bicgstab": sa.BiCGStab, "minres": sa.MinRes}[solver]
    ip, ix, d, rhs, A, P = _handles(sa, name, dt)
    n = rhs.size
    tol = tol_of(dt)
    max_iter = max_iter_of(solver, name, dtname)
    o = checker_run(solver, name, dtname)
    prefix = trace_prefix(solver, name, dtname)
    assert o.status == kp.OK and 2 * o.its <= max_iter and prefix >= 1
    out = {}
    for mode in ("literal", "fused"):
        s = cls.new(A, n); s.set_mode(mode); s.set_trace(max_iter + 1)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace(), _true_res(ip, ix, d, rhs, x))
    (sl, il, rl, xl, tl, true_l), (sf, itf, rf, xf, tf, true_f) = out["literal"], out["fused"]
    print("%s+fsai %s %s: literal its %s (checker %d) res %s (checker %.3e) true %.3e rows %d; fused its %s res %s true %.3e rows %d; prefix %d"
          % (solver, name, dtname, il, o.its, rl, o.res, true_l, len(tl), itf, rf, true_f, len(tf), prefix))
    rtol, atol = gpu_tols(dt)
    # literal against the checker
    assert sl == kp.OK and abs(il - o.its) <= _margin(o.its)
    k = min(prefix, len(tl), len(o.trace))
    assert k >= 1 and _cg_trace_close(tl[:k], o.trace[:k], rtol=rtol, atol=atol)
    assert rl <= tol and true_l <= 10 * tol
    # fused against literal
    assert sf == kp.OK and abs(itf - il) <= _margin(il)
    k = min(prefix, len(tf), len(tl))
    assert k >= 1 and _cg_trace_close(tf[:k], tl[:k], rtol=rtol, atol=atol)
    assert rf <= tol and true_f <= 10 * tol
    # without a trace buffer (lazy polling) and on device vectors the fused solve returns the same bits
    s = cls.new(A, n)
    x2 = np.zeros(n, dt)
    assert _run(sa, s, P, rhs, x2, max_iter, tol)[:2] == (sf, itf) and np.array_equal(x2, xf)
    d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n, dt))
    assert _run(sa, s, P, d_rhs, d_x, max_iter, tol)[:2] == (sf, itf) and np.array_equal(d_x.to_numpy(), xf)


@pytest.mark.parametrize("name,dt", [(name, dt) for name in SYSTEMS for dt in ALL], ids=_ids)
def test_gmres_literal_follows_the_checker_and_fused_follows_literal(sa, name, dt):
    """tests/test_gpu_ilu.py::test_gmres_literal_follows_the_checker_and_fused_follows_literal with M = FSAI(power 1); the trace
    rows over the prefix that tests/test_fsai_cpu.py derives by the same rule as GMRES_TRACE_ROWS."""
    dtname = np.dtype(dt).name
    ip, ix, d, rhs, A, P = _handles(sa, name, dt)
    n = rhs.size
    tol = tol_of(dt)
    m = GMRES_RESTART
    max_iter = max_iter_of("gmres", name, dtname)
    o = checker_run("gmres", name, dtname)
    rows = trace_prefix("gmres", name, dtname)
    assert o.status == ref.OK and 2 * o.its <= max_iter and rows >= 1
    out = {}
    for mode in ("literal", "fused"):
        s = sa.GMRES.new(A, n, m); s.set_mode(mode); s.set_trace(max_iter)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace(), _true_res(ip, ix, d, rhs, x))
    (sl, il, rl, xl, tl, true_l), (sf, itf, rf, xf, tf, true_f) = out["literal"], out["fused"]
    want = gmres_trace_array(o.trace)
    err = np.max(np.abs(xl - o.x))
    print("gmres+fsai %s %s: literal its %d (checker %d) res %.3e (checker %.3e) true %.3e max|x - checker| %.3e; fused its %d res %.3e true %.3e max|dx| %.3e; rows %d"
          % (name, dtname, il, o.its, rl, o.res, true_l, err, itf, rf, true_f, np.max(np.abs(xf - xl)), rows))
    # literal against the checker
    assert sl == o.status == ref.OK
    assert abs(il - o.its) <= _margin(o.its)
    assert tl.shape == (il, 8) and np.array_equal(tl[:, 0], np.arange(1, il + 1))
    assert rl <= tol and true_l <= 10 * tol
    k = min(rows, il, o.its)
    if is_single(dt):
        assert gm_trace_close(tl[:1], want[:1], rtol=1e-5, atol=1e-8)
        assert err < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
    else:
        assert gm_trace_close(tl[:k], want[:k], rtol=1e-9, atol=1e-12)
        assert err <= 1e-7 * max(1.0, np.max(np.abs(o.x)))
        assert il == o.its and np.isclose(rl, o.res, rtol=1e-9, atol=1e-12)
    # fused against literal
    assert sf == sl == ref.OK
    assert abs(itf - il) <= _margin(il)
    assert rf <= tol and true_f <= 10 * tol
    assert tf.shape == (itf, 8) and np.array_equal(tf[:, 0], np.arange(1, itf + 1))
    k = min(rows, itf, il)
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


# ------------------------------------------------------------------------------------------------ 7. the factor views
@pytest.mark.parametrize("dt", [F64, C32], ids=_ids)
def test_factor_views(sa, dt):
    """P.G and P.GH are ordinary handles: read through sprs_csr_read they are P.factor() and its stated adjoint, they report a
    stream format, and multiplying by them has the bits of the row fold."""
    from _amg_ref import Ops, spmv
    ip, ix, d, rhs, A, P = _handles(sa, "cg", dt, 2)
    n = rhs.size
    f = factor_of("cg", np.dtype(dt).name, 2)
    G, GH = P.G, P.GH
    gp, gx, gv = G.to_host()
    assert np.array_equal(gp, f.ip) and np.array_equal(gx, f.ix) and np.array_equal(bits(gv), bits(f.val))
    hp, hx, hv = GH.to_host()
    wp, wx, wv = fr.adjoint(f.ip, f.ix, f.val)
    assert np.array_equal(hp, wp) and np.array_equal(hx, wx) and np.array_equal(bits(hv), bits(wv))
    assert G.shape == GH.shape == (n, n) and G.nnz() == GH.nnz() == f.ix.size
    print("fsai(2) cg %s: stream formats G %s, GH %s" % (np.dtype(dt).name, G.stream_format(), GH.stream_format()))
    assert G.stream_format()[0] in (0, 1, 2) and GH.stream_format()[0] in (0, 1, 2)
    y = np.zeros(n, dt)
    G.mul_vec(rhs, y)
    assert np.array_equal(bits(y), bits(spmv(Ops(dt), f.ip, f.ix, f.val, rhs)))
    G.close(); GH.close()                                                         # a view's close leaves the factor alone
    out = np.zeros(n, dt)
    P.mul_vec(rhs, out)
    assert np.array_equal(bits(out), bits(applier("cg", np.dtype(dt).name, 2)(rhs)))
    from sprsolve_amd import _lib
    h = C.c_void_p()
    assert _lib.lib().sprs_fsai_factor(P.h, 2, C.byref(h)) == _lib.INVALID_ARGUMENT
    assert _lib.lib().sprs_fsai_factor(None, 0, C.byref(h)) == _lib.INVALID_ARGUMENT
