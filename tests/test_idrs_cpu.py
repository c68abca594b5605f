"""IDR(s) without a GPU: the C ABI and the Python mirror exist, null handles are refused, and the checker of the GPU tests
(tests/_idrs_ref.py) is itself checked: against a dense solve, against a plain BiCGStab (IDR(1) with P = rhs / |rhs| and kappa = 0
is BiCGStab), on finite termination, and on how far a change of summation order moves it — the margins the GPU tests allow.

Observed with this checker (x0 = 0, 8 summation orders each, 3 on the 8640-row grid; every dot product is summed in double, so
an order moves the scalars by 1e-16 and the single-precision start norm by 1e-7): the step counts move by at most 5 on the
convection-dominated (24, 22) grid (margin 18 to 23) and by at most 2 elsewhere, and the true residual stays below 1.01 tol.  The harder grids are f64 / c64 inputs only: in f32 their true residual drifts from the
recursive one (IDR's residual gap)."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_ref as ref  # noqa: E402
import _idrs_ref as idr  # noqa: E402

F64, C64, F32, C32 = idr.F64, idr.C64, idr.F32, idr.C32
NAMES = sorted(["sprs_idrs_%s_%s" % (f, s) for f in ("create", "solve", "precond_solve", "solve_dev") for s in "dzsc"]
               + ["sprs_%s_idrs_%s_%s" % (pc, f, s) for pc in ("ilu0", "amg", "fsai") for f in ("solve", "solve_dev") for s in "dzsc"]
               + ["sprs_idrs_destroy"])


@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_abi_and_binding_exist(L):
    src = open(os.path.join(ROOT, "include", "sprsolve_hip.h")).read()
    m = re.search(r"#define\s+SPRS_IDRS_MAX_S\s+(\d+)", src)
    assert m and int(m.group(1)) == idr.MAX_S == 8
    assert re.search(r"SPRS_SOLVER_IDRS\s*=\s*7\b", src)
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(sprs_[a-z0-9_]+)\s*\(", src))
    assert len(NAMES) == 41 and sorted(n for n in declared if "_idrs_" in n) == NAMES
    assert re.search(r"typedef\s+struct\s+sprs_idrs\s+sprs_idrs\s*;", src)
    from sprsolve_amd import _lib
    assert _lib.SOLVER_IDRS == 7 and _lib.IDRS_MAX_S == 8
    for name in NAMES:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
    import sprsolve_amd
    assert callable(sprsolve_amd.IDRS.new) and callable(sprsolve_amd.IDRS.solve) and callable(sprsolve_amd.IDRS.precond_solve)


def test_null_handles_are_rejected(L):
    out = C.c_void_p()
    for s in "dzsc":
        assert getattr(L, "sprs_idrs_create_" + s)(None, 4, 2, C.byref(out)) == 7 and not out.value
        assert getattr(L, "sprs_idrs_solve_" + s)(None, None, 4, None, 4, 10, 1e-8, None, None) == 7
        for f in ("idrs_precond_solve_", "idrs_solve_dev_", "ilu0_idrs_solve_", "amg_idrs_solve_dev_", "fsai_idrs_solve_"):
            assert getattr(L, "sprs_" + f + s)(None, None, None, 4, None, 4, 10, 1e-8, None, None) == 7
    assert L.sprs_idrs_destroy(None) == 0
    assert L.sprs_solver_set_mode(None, 7, 1) == 7


def _true_res(A, rhs, x):
    """|rhs - A x| / |rhs| formed in double."""
    W = np.complex128 if np.dtype(x.dtype).kind == "c" else np.float64
    D = ref.dense(A[0], A[1], A[2].astype(W))
    return float(np.linalg.norm(rhs.astype(W) - D @ x.astype(W)) / np.linalg.norm(rhs.astype(W)))


def test_shadow_space_is_orthonormal():
    for dt in (F64, C64, F32, C32):
        P = idr.shadow(132, 8, dt)
        eps = np.finfo(idr.real_of(dt)).eps
        assert P.dtype == np.dtype(dt) and np.max(np.abs(P.conj() @ P.T - np.eye(8))) <= 64 * eps


@pytest.mark.parametrize("dt", [F64, C64, F32, C32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("s", [1, 4, 8])
def test_checker_against_dense_solve(dt, s):
    name = "csg9x8" if np.dtype(dt).kind == "c" else "cd12x11"
    ip, ix, d, rhs, diag = idr.system(name, dt)
    n = rhs.size
    W = np.complex128 if np.dtype(dt).kind == "c" else np.float64
    xs = np.linalg.solve(ref.dense(ip, ix, d.astype(W)), rhs.astype(W))
    tol = idr.tol_of(dt)
    for pc in (None, diag):
        o = idr.idrs((ip, ix, d), rhs, np.zeros(n, dt), 400, tol, s=s, precond_diag=pc)
        err = np.max(np.abs(o.x - xs)) / np.max(np.abs(xs))
        print("%s s=%d %s: its %d res %.3e max|x - x*| / max|x*| %.3e" % (np.dtype(dt).name, s, "jacobi" if pc is not None else "none", o.its, o.res, err))
        assert o.status == idr.OK and o.x.dtype == np.dtype(dt) and o.res <= tol
        assert len(o.trace) == o.its and len(o.rns) == o.its + 1
        assert err <= 200 * tol                            # cond(A) < 100 on both grids
    # a non-zero start is honoured: from the solution rounded to the dtype the first test ends the solve
    o = idr.idrs((ip, ix, d), rhs, xs.astype(dt), 400, 1e-4 if tol > 1e-6 else 1e-9, s=s)
    assert o.status == idr.OK and o.its == 0


def _bicgstab_plain(A, rhs, iters):
    """BiCGStab from x = 0 with the shadow vector r_0, in double: |r| after each of `iters` iterations."""
    r = rhs.copy(); r0 = r.copy()
    rho = alpha = w = 1.0
    v = np.zeros_like(r); p = np.zeros_like(r)
    out = []
    for _ in range(iters):
        rho_new = r0 @ r
        beta = (rho_new / rho) * (alpha / w)
        p = r + beta * (p - w * v)
        v = A @ p
        alpha = rho_new / (r0 @ v)
        sv = r - alpha * v
        t = A @ sv
        w = (t @ sv) / (t @ t)
        r = sv - w * t
        rho = rho_new
        out.append(float(np.linalg.norm(r)))
    return out


def test_idr1_is_bicgstab():
    ip, ix, d, rhs, _ = idr.system("cd12x11", F64)
    n = rhs.size
    P = (rhs / np.linalg.norm(rhs)).reshape(1, n)
    o = idr.idrs((ip, ix, d), rhs, np.zeros(n), 12, 1e-30, s=1, kappa=0.0, P=P)
    mine = o.rns[2:13:2]                                   # |r| after each cycle of two products
    theirs = _bicgstab_plain(ref.dense(ip, ix, d), rhs, 6)
    print("IDR(1):   ", mine, "\nBiCGStab: ", theirs)
    assert len(mine) == 6
    np.testing.assert_allclose(mine, theirs, rtol=1e-9, atol=0)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 7])
def test_finite_termination(n):
    rng = np.random.default_rng(100 + n)
    A = rng.standard_normal((n, n)) + 3.0 * np.eye(n)
    rhs = rng.standard_normal(n)
    xs = np.linalg.solve(A, rhs)
    for s in sorted({1, min(2, n), n}):
        bound = n + math.ceil(n / s)
        o = idr.idrs(A, rhs, np.zeros(n), bound, 1e-12, s=s)
        print("n=%d s=%d: its %d of %d, res %.3e" % (n, s, o.its, bound, o.res))
        assert o.status == idr.OK and o.its <= bound and o.res <= 1e-12
        assert np.max(np.abs(o.x - xs)) <= 1e-9 * max(1.0, np.max(np.abs(xs)))


def test_events_of_the_checker():
    ip, ix, d, rhs, _ = idr.system("cd12x11", F64)
    n = rhs.size
    full = idr.idrs((ip, ix, d), rhs, np.zeros(n), 400, 1e-10, s=4)
    o = idr.idrs((ip, ix, d), np.zeros(n), np.ones(n), 400, 1e-10, s=4)
    assert o.status == idr.OK and o.its == 0 and not np.any(o.x)
    o = idr.idrs((ip, ix, d), rhs, np.zeros(n), 7, 1e-10, s=4)       # mid-cycle: the first seven steps of the full solve
    assert o.status == idr.INSUFFICIENT_ITER and o.its == 7 and o.trace == full.trace[:7]
    o = idr.idrs((ip, ix, d), rhs, np.zeros(n), 0, 1e-10, s=4)
    assert o.status == idr.INSUFFICIENT_ITER and o.its == 0 and not np.any(o.x)
    Z = np.zeros((2, 2)); Z[1, 1] = 1.0                                # a zero row and column: singular
    o = idr.idrs(Z, np.array([1.0, 1.0]), np.zeros(2), 50, 1e-10, s=1)
    assert o.status == idr.BREAKDOWN


@pytest.mark.parametrize("case", idr.FOLLOW + idr.HARDER + idr.SHAPES,
                         ids=lambda c: "%s-%s-s%d-%s" % (c[0], np.dtype(c[1]).name, c[2], "jacobi" if c[3] else "none"))
def test_margins_hold_under_another_summation_order(case):
    """What the GPU tests allow between the library and this checker — max(5, its // 4) steps, a true residual of 10 tol — holds
    between the checker and itself with every sum taken in a permuted order."""
    name, dt, s, pc = case
    ip, ix, d, rhs, diag = idr.system(name, dt)
    n = rhs.size
    tol = idr.tol_of(dt)
    run = lambda order: idr.idrs((ip, ix, d), rhs, np.zeros(n, dt), 2000, tol, s=s, precond_diag=diag if pc else None, order=order)
    base = run(None)
    assert base.status == idr.OK and base.res <= tol
    worst_steps, worst_true = 0, _true_res((ip, ix, d), rhs, base.x)
    for seed in range(3 if n > 2000 else 8):
        o = run(np.random.default_rng(seed).permutation(n))
        assert o.status == idr.OK and o.res <= tol
        worst_steps = max(worst_steps, abs(o.its - base.its))
        worst_true = max(worst_true, _true_res((ip, ix, d), rhs, o.x))
    print("%s: its %d, moved by <= %d (margin %d); true residual <= %.2f tol" % (case[0], base.its, worst_steps, idr.margin(base.its), worst_true / tol))
    assert worst_steps <= idr.margin(base.its)
    assert worst_true <= 10 * tol
