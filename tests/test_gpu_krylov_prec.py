"""BiCGStab and MINRES preconditioned by an applied handle (ILU(0), its Jacobi sweeps, AMG) on the GPU
(sprs_{ilu0,amg}_{bicgstab,minres}_solve*, csrc/bicgstab.hip, csrc/minres.hip) against the checker of tests/_krylov_prec_ref.py:
the literal mode follows the checker and the fused mode follows the literal mode over the trace prefix that
tests/test_krylov_prec_cpu.py derives, at the tolerances tests/test_gpu_ilu.py uses for CG; the InvalidPreconditioner end of MINRES, the
restart branch of BiCGStab under an applied M, the refusals, and the untouched diagonal path on the same solver handle.

The checker's counts (tests/test_krylov_prec_cpu.py) stand behind every max_iter, each at least twice its count."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _krylov_prec_ref as kp  # noqa: E402
from test_amg_cpu import system_of  # noqa: E402
from test_gpu_ilu import _cg_trace_close, _margin, _run, _true_res  # noqa: E402
from test_ilu_cpu import ALL, C32, C64, F32, F64, is_single, tol_of  # noqa: E402,F401
from test_krylov_prec_cpu import (BICG_GPU_CASES, INDEFINITE_MINRES, MINRES_GPU_CASES, applier, checker_run, gpu_tols, max_iter_of,  # noqa: E402
                                  restart_cases, restart_problem, trace_prefix)

pytestmark = pytest.mark.gpu

_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


def _prec(sa, A, kind):
    if kind == "amg":
        return sa.AMG.new(A)
    if kind == "ilu":
        return sa.ILU0.new(A)
    assert kind.startswith("ilu_s")
    return sa.ILU0.new(A, sweeps=int(kind[5:]))


def _handles(sa, name, dt, kind):
    ip, ix, d, rhs = system_of(name, np.dtype(dt).name)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    return ip, ix, d, rhs, A, _prec(sa, A, kind)


def _jacobi(sa, ip, ix, d):
    n = ip.size - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    return sa.DiagPrecond.new(d[rows == ix].real.astype(np.float32 if is_single(d.dtype) else np.float64).copy(), t_dtype=d.dtype)


def _follows(sa, solver, cls, name, dt, kind):
    """Literal against the checker, fused against literal, over the derived trace prefix; then the fused solve without a trace buffer
    and on device vectors."""
    dtname = np.dtype(dt).name
    ip, ix, d, rhs, A, P = _handles(sa, name, dt, kind)
    n = rhs.size
    tol = tol_of(dt)
    max_iter = max_iter_of(solver, name, dtname, kind)
    o = checker_run(solver, name, dtname, kind)
    prefix = trace_prefix(solver, name, dtname, kind)
    assert o.status == kp.OK and 2 * o.its <= max_iter and prefix >= (5 if np.dtype(dt) == np.dtype(F64) else 1)
    out = {}
    for mode in ("literal", "fused"):
        s = cls.new(A, n); s.set_mode(mode); s.set_trace(max_iter + 1)
        x = np.zeros(n, dt)
        st, its, res = _run(sa, s, P, rhs, x, max_iter, tol)
        out[mode] = (st, its, res, x, s.trace(), _true_res(ip, ix, d, rhs, x))
    (sl, il, rl, xl, tl, true_l), (sf, itf, rf, xf, tf, true_f) = out["literal"], out["fused"]
    print("%s+%s %s %s: literal its %s (checker %d) res %s (checker %.3e) true %.3e rows %d; fused its %s res %s true %.3e rows %d; prefix %d"
          % (solver, kind, name, dtname, il, o.its, rl, o.res, true_l, len(tl), itf, rf, true_f, len(tf), prefix))
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
    return itf


# ------------------------------------------------------------------------------------------------ 1. BiCGStab
@pytest.mark.parametrize("name,dt,kind", BICG_GPU_CASES, ids=_ids)
def test_bicgstab_literal_follows_the_checker_and_fused_follows_literal(sa, name, dt, kind):
    """cd24x20 (480 rows) in all four types under ILU0, ILU0(sweeps=3) and AMG; cd64x64 (4096 rows) under AMG: level 0 lies above
    the 1024-row tail, so multi-workgroup level kernels run between the solver's; p3_12x11x10 under the exact ILU(0): batched and
    per-level launches between K1 .. K5."""
    itf = _follows(sa, "bicgstab", sa.BiCGStab, name, dt, kind)
    if name == "cd24x20":
        jac = checker_run("bicgstab", name, np.dtype(dt).name, "jacobi").its
        assert itf < jac                                                           # fewer iterations than Jacobi needs


# ------------------------------------------------------------------------------------------------ 2. MINRES
@pytest.mark.parametrize("name,dt,kind", MINRES_GPU_CASES, ids=_ids)
def test_minres_literal_follows_the_checker_and_fused_follows_literal(sa, name, dt, kind):
    _follows(sa, "minres", sa.MinRes, name, dt, kind)


def test_minres_invalid_preconditioner_event(sa):
    """MINRES + AMG on the indefinite grid: the rule of minres.rs:279-287 fires at iteration 4 with re(b2) = -0.16, in both modes;
    iteration, re(b2) and x against the checker at the tolerances of tests/test_gpu_ilu.py::test_cg_invalid_preconditioner_event."""
    ip, ix, d, rhs, A, P = _handles(sa, "indefinite", F64, "amg")
    n = rhs.size
    o = kp.minres(ip, ix, d, rhs, np.zeros(n), 50, 1e-10, prec=applier("indefinite", "float64", "amg"))
    assert (o.status, o.its) == (kp.INVALID_PRECOND, INDEFINITE_MINRES[0])
    for mode in ("fused", "literal"):
        s = sa.MinRes.new(A, n); s.set_mode(mode)
        x = np.zeros(n)
        with pytest.raises(sa.error.InvalidPreconditioner) as ei:
            s.precond_solve(P, rhs, x, 50, 1e-10)
        m = re.match(r"beta_(\d+) \[(.+)\] is not positive", ei.value.msg)
        print("minres+amg indefinite %s: %s (checker: its %d, re(b2) %r); max|x - checker| %.3e" % (mode, ei.value.msg, o.its, o.res, np.max(np.abs(x - o.x))))
        assert m and int(m.group(1)) == o.its
        assert np.isclose(float(m.group(2)), o.res, rtol=1e-9, atol=1e-12)
        assert np.allclose(x, o.x, rtol=1e-9, atol=1e-12), mode


# ------------------------------------------------------------------------------------------------ 3. the restart branch
def test_bicgstab_restart_branch_under_an_applied_preconditioner(sa):
    """bicg_stab.rs:131-145 with an applied M (the cases tests/test_krylov_prec_cpu.py found: `restart_converges` under one Jacobi
    sweep of ILU(0), in one copy and in 700): rho == 0 exactly at its = 1, the host rebuilds r, r0 and rho and re-enters with
    K1(mode 1); both modes follow the checker through it (tests/test_gpu_parity.py::test_bicgstab_restart_branch's comparisons)."""
    cases = restart_cases()
    assert len(cases) >= 2
    for case in cases:
        _restart_case(sa, case)


def _restart_case(sa, case):
    name, copies, kind, events, want_status, want_its = case
    ip, ix, d, b, max_iter, tol = restart_problem(name, copies)
    n = b.size
    f_kind, k = kind[:5], int(kind[5:])
    assert f_kind == "ilu_s"
    import _ilu_ref
    import _ilu_sweeps_ref
    M = _ilu_sweeps_ref.Sweeps(ip, ix, _ilu_ref.ilu0(ip, ix, d).val, k)
    o = kp.bicgstab(ip, ix, d, b, np.zeros(n), max_iter, tol, prec=M)
    assert tuple(o.events) == events and (o.status, o.its) == (want_status, want_its) == (kp.OK, 4)
    A = sa.HipCsr.new((n, n), ip, ix, d)
    P = sa.ILU0.new(A, sweeps=k)
    for mode in ("fused", "literal"):
        s = sa.BiCGStab.new(A, n); s.set_mode(mode); s.set_trace(8)
        x = np.zeros(n)
        st, its, res = _run(sa, s, P, b, x, max_iter, tol)
        tr = s.trace()
        print("restart %s x%d %s %s: its %s res %s rows %d; checker its %d res %.3e" % (name, copies, kind, mode, its, res, len(tr), o.its, o.res))
        assert (st, its) == (o.status, o.its)
        # the restart replaces rho by |A x - b|^2 at its = 1 — visible in the trace
        assert np.isclose(tr[1][2], o.trace[1][2], rtol=1e-12) and np.isclose(tr[1][2], tr[1][1] ** 2, rtol=1e-12)
        assert np.allclose(x, o.x, rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_wrong_handle_is_refused_by_the_four_new_entry_families(sa):
    from sprsolve_amd import _lib
    ip, ix, d, rhs = system_of("cd24x20", "float64")
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    ip32, ix32, d32, _ = system_of("cd24x20", "float32")
    A32 = sa.HipCsr.new((n, n), ip32, ix32, d32)
    ips, ixs, ds, rs = system_of("tri300", "float64")
    As = sa.HipCsr.new((rs.size, rs.size), ips, ixs, ds)
    ctx2 = sa.Context(0)
    A2 = sa.HipCsr.new((n, n), ip, ix, d, ctx=ctx2)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for pfx, mk in (("ilu0", sa.ILU0.new), ("amg", sa.AMG.new)):
        P, P32, Psmall, Pother = mk(A), mk(A32), mk(As), mk(A2)
        for sname, cls in (("bicgstab", sa.BiCGStab), ("minres", sa.MinRes)):
            x = np.zeros(n)
            for mode in ("fused", "literal"):
                s = cls.new(A, n); s.set_mode(mode)
                with pytest.raises(ValueError):
                    s.precond_solve(P32, rhs, x, 10, 1e-10)                       # another scalar type
                with pytest.raises(ValueError):
                    s.precond_solve(Pother, rhs, x, 10, 1e-10)                    # a handle of a matrix on another context
                with pytest.raises(sa.error.DimensionMismatch):
                    s.precond_solve(Psmall, rhs, x, 10, 1e-10)                    # another matrix, of another size
                d_rhs = sa.DevVec.from_numpy(rhs); d_x = sa.DevVec.from_numpy(np.zeros(n))
                with pytest.raises(sa.error.DimensionMismatch):
                    s.precond_solve(Psmall, d_rhs, d_x, 10, 1e-10)
                assert not np.any(d_x.to_numpy())
            assert not np.any(x)
            its = C.c_size_t(); res = C.c_double()
            s = cls.new(A, n)
            fn = getattr(_lib.lib(), "sprs_%s_%s_solve_d" % (pfx, sname))
            assert fn(s.h, None, p(rhs.copy()), n, p(x), n, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INVALID_ARGUMENT
            assert fn(s.h, P.h, p(rhs.copy()), n - 1, p(x), n, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INCOMPATIBLE_RHS_SIZE
            assert fn(s.h, P.h, p(rhs.copy()), n, p(x), n + 1, 10, 1e-10, C.byref(its), C.byref(res)) == _lib.INCOMPATIBLE_X_SIZE
            assert not np.any(x)


def test_csminres_refuses_a_preconditioner(sa):
    ip, ix, d, rhs, A, P = _handles(sa, "cg", F64, "amg")
    n = rhs.size
    s = sa.CSMinRes.new(A, n)
    x = np.zeros(n)
    for M in (P, sa.ILU0.new(A), _jacobi(sa, ip, ix, d)):
        with pytest.raises(TypeError):
            s.precond_solve(M, rhs, x, 10, 1e-10)
    assert not np.any(x)
    its, res = s.solve(rhs, x, 200, 1e-10)                                        # ... and still solves without one
    assert res <= 1e-10


# ------------------------------------------------------------------------------------------------ 5. buffer roles
@pytest.mark.parametrize("kind", ["ilu", "amg"])
def test_diagonal_and_plain_solves_are_the_same_before_and_after_an_applied_solve(sa, kind):
    """An applied solve uses the 7-vector layout of the preconditioned branch; the unpreconditioned solve on the same handle uses five
    and lets p alias y.  Status, count and bits of x of `solve` and of `precond_solve(DiagPrecond)` do not depend on what the handle ran before."""
    ip, ix, d, rhs, A, P = _handles(sa, "cd24x20", F64, kind)
    n = rhs.size
    J = _jacobi(sa, ip, ix, d)
    s = sa.BiCGStab.new(A, n)

    def both():
        xj = np.zeros(n); xn = np.zeros(n)
        a = _run(sa, s, J, rhs, xj, 200, 1e-10)[:2]
        its, res = s.solve(rhs, xn, 200, 1e-10)
        return a, xj, its, xn

    a0, xj0, i0, xn0 = both()
    xa = np.zeros(n)
    assert _run(sa, s, P, rhs, xa, 60, 1e-10)[0] == kp.OK
    a1, xj1, i1, xn1 = both()
    assert a0 == a1 and a0[0] == kp.OK and np.array_equal(xj0, xj1)
    assert i0 == i1 and np.array_equal(xn0, xn1)
    xb = np.zeros(n)
    assert _run(sa, s, P, rhs, xb, 60, 1e-10)[0] == kp.OK and np.array_equal(xa, xb)   # ... and the applied solve repeats its bits
