"""BiCGStab and MINRES with an applied preconditioner (ILU(0), its Jacobi sweeps, AMG) without a GPU: the checker of
tests/_krylov_prec_ref.py is tied to the CPU oracle, its iteration counts are pinned, and everything tests/test_gpu_krylov_prec.py
compares against is derived here: the checker's results (computed once, shared, read-only), the trace prefix the GPU may be held
to, the largest imaginary part of MINRES' conj(v).M v on the complex fixtures, the InvalidPreconditioner end on an indefinite
matrix, and the restart cases of tests/golden/branch_kat.json that an applied M still drives into BiCGStab's restart branch.
The 32 entry points sprs_{ilu0,amg}_{bicgstab,minres}_solve[_dev]_{d,z,s,c} exist in the header, the library and the binding."""
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _amg_ref as amg  # noqa: E402
import _golden as G  # noqa: E402
import _ilu_ref as ref  # noqa: E402
import _ilu_sweeps_ref as sweeps_ref  # noqa: E402
import _krylov_prec_ref as kp  # noqa: E402
from test_amg_cpu import hierarchy_of, system_of  # noqa: E402
from test_ilu_cpu import ALL, C32, C64, F32, F64, is_single, tol_of  # noqa: E402,F401

_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name

SWEEPS = 3                                                    # the Jacobi-sweep handle of the GPU cases: ILU0(sweeps=3)
KINDS = ("ilu", "ilu_s3", "amg")

# the checker's counts, x0 = 0, f64 / c64 at tol 1e-10 and f32 / c32 at 1e-5: (Jacobi, ILU(0), AMG)
BICG_COUNTS = {
    "cd24x20": {"float64": (47, 14, 9), "complex128": (49, 15, 9), "float32": (34, 9, 5), "complex64": (33, 9, 5)},
    "cd64x64": {"float64": (122, 33, 13)},
    "cg": {"float64": (47, 14, 9), "complex128": (31, 9, 14)},
    "p3_12x11x10": {"float64": (None, 14, None)},             # (the matrix of "cg" under system_of's seeded right-hand side; ILU(0) only)
}
BICG_SWEEPS_COUNTS = {"float64": 20, "complex128": 19, "float32": 13, "complex64": 13}     # cd24x20, ILU0(sweeps=3)
MINRES_COUNTS = {"float64": (62, 20, 14), "complex128": (40, 14, 21), "float32": (22, 7, 6), "complex64": (22, 7, 12)}   # system "cg"
# iteration and re(b2) of MINRES + AMG on system "indefinite" (tests/test_amg_cpu.py::indefinite_grid): InvalidPreconditioner
INDEFINITE_MINRES = (4, -0.1613)
# largest im(b2) / (eps re(b2)) seen on the complex fixtures of the GPU test (c64, ILU(0)); the reference's limit is 1
IMAG_RATIO_LIMIT = 0.5


# ------------------------------------------------------------------------------------------------ what the GPU test shares
@functools.lru_cache(maxsize=None)
def applier(name, dtname, kind):
    """The callable M of a named system: "jacobi", "ilu" (exact), "ilu_s<k>" (k Jacobi sweeps), "amg", or None for "none"."""
    ip, ix, d, _ = system_of(name, dtname)
    if kind == "none":
        return None
    if kind == "jacobi":
        return ref.jacobi(ip, ix, d)
    if kind == "amg":
        return amg.Applier(hierarchy_of(name, dtname))
    f = ref.ilu0(ip, ix, d)
    assert f.status == ref.OK
    if kind == "ilu":
        return ref.Applier(ip, ix, f.val)
    assert kind.startswith("ilu_s")
    return sweeps_ref.Sweeps(ip, ix, f.val, int(kind[5:]))


def max_iter_of(solver, name, dtname, kind):
    """At least twice the checker's count (tests/test_gpu_cg.py's rule)."""
    if solver == "minres":
        return 2 * MINRES_COUNTS[dtname][{"jacobi": 0, "ilu": 1, "amg": 2}[kind]] + 2
    if kind == "ilu_s3":
        return 2 * BICG_SWEEPS_COUNTS[dtname]
    return 2 * BICG_COUNTS[name][dtname][{"jacobi": 0, "none": 0, "ilu": 1, "amg": 2}[kind]] + 2


@functools.lru_cache(maxsize=None)
def checker_run(solver, name, dtname, kind, sums="numpy"):
    ip, ix, d, rhs = system_of(name, dtname)
    dt = np.dtype(dtname).type
    o = getattr(kp, solver)(ip, ix, d, rhs, np.zeros(rhs.size, dt), max_iter_of(solver, name, dtname, kind), tol_of(dt),
                            prec=applier(name, dtname, kind), sums=sums)
    o.x.setflags(write=False); o.trace.setflags(write=False)
    return o


def gpu_tols(dt):
    """(rtol, atol) of a trace comparison on the GPU: tests/test_gpu_ilu.py's for CG."""
    return (1e-5, 1e-8) if is_single(dt) else (1e-9, 1e-12)


def cx_rows(t):
    """tests/test_gpu_ilu.py::_cg_trace_close's view of 8-double rows: two reals and three complex numbers."""
    t = np.atleast_2d(t)
    return np.concatenate([t[:, :2].astype(complex), t[:, 2::2] + 1j * t[:, 3::2]], axis=1)


def rows_close(a, b, rtol, atol):
    """-> the number of leading rows of a and b that agree."""
    k = min(len(a), len(b))
    bad = np.nonzero(~np.isclose(cx_rows(a[:k]), cx_rows(b[:k]), rtol=rtol, atol=atol).all(axis=1))[0]
    return int(bad[0]) if bad.size else k


@functools.lru_cache(maxsize=None)
def trace_prefix(solver, name, dtname, kind):
    """The trace rows the GPU test may compare (the rule of tests/test_ilu_cpu.py, GMRES_TRACE_ROWS): the leading rows on which the
    checker against itself with its sums taken pairwise holds a TENTH of the GPU tolerance.  Past them a change of summation
    order alone moves the scalars by more than that, and the GPU's order is a third one."""
    rtol, atol = gpu_tols(np.dtype(dtname).type)
    a, b = checker_run(solver, name, dtname, kind), checker_run(solver, name, dtname, kind, "pairwise")
    return rows_close(a.trace, b.trace, rtol / 10, atol / 10)


def _dense_restart_case(c, copies):
    import scipy.sparse as sp
    M = sp.block_diag([sp.csr_matrix(np.array(c["A"], float))] * copies, format="csr")
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.copy(), np.tile(np.array(c["b"], float), copies)


@functools.lru_cache(maxsize=None)
def restart_cases():
    """The `restart` cases of tests/golden/branch_kat.json (one copy, and 700 on a block diagonal: more than one workgroup) under
    ILU0(sweeps = 1, 2, 3) and AMG (the defaults): those where the checker with the applied M takes the restart branch
    (bicg_stab.rs:131-145) -> ((case name, copies, kind, restart iterations, checker status, checker its), ...)."""
    found = []
    for c in G.load("branch_kat.json")["restart"]:
        for copies in (1, 700):
            ip, ix, d, b = _dense_restart_case(c, copies)
            for kind, M in restart_appliers(ip, ix, d):
                for sums in ("numpy", "pairwise"):
                    o = kp.bicgstab(ip, ix, d, b, np.zeros_like(b), c["max_iter"], c["tol"], prec=M, sums=sums)
                    if not o.events:
                        break
                else:                                          # the branch is taken whatever the summation order
                    o = kp.bicgstab(ip, ix, d, b, np.zeros_like(b), c["max_iter"], c["tol"], prec=M)
                    found.append((c["name"], copies, kind, tuple(o.events), o.status, o.its))
    return tuple(found)


def restart_appliers(ip, ix, d):
    out = []
    f = ref.ilu0(ip, ix, d)
    if f.status == ref.OK:
        out += [("ilu_s%d" % k, sweeps_ref.Sweeps(ip, ix, f.val, k)) for k in (1, 2, 3)]
    H = amg.build(ip, ix, d)
    if H.status == amg.OK:
        out.append(("amg", amg.Applier(H)))
    return out


def restart_problem(name, copies):
    c = [c for c in G.load("branch_kat.json")["restart"] if c["name"] == name][0]
    return _dense_restart_case(c, copies) + (c["max_iter"], c["tol"])


# ------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("case", [c for c in G.load("solver_kat.json")["cases"] if c["precond"] is not None], ids=lambda c: c["name"])
def test_checker_with_a_diagonal_follows_the_oracle(oracle, case):
    """The reference's own preconditioned problems (tests/test_complex_solve.rs), the oracle's diagonal against the checker's
    callable.  Both end Ok, and the first 10 trace rows agree at rtol 1e-9 / atol 1e-12.  The iteration counts are compared within
    max(5, its / 4), tests/test_gpu_cg.py's margin between two summation orders, not for equality: these problems ask for
    1e-22, far below what f64 resolves, so the count is decided by rounding — the oracle's serial folds need 103 / 112 / 40
    iterations, the checker 102 / 118 / 40 with numpy's sums and 103 / 115 / 40 with pairwise ones, and the three traces part
    from row 11 (BiCGStab) or 31 (MINRES) on."""
    p = G.solver_problem(case)
    dg = p["diag"]
    dinv = (dg.dtype.type(1) / dg).astype(dg.dtype)
    M = lambda v: (v * dinv).astype(v.dtype)
    x0 = np.zeros_like(p["rhs"])
    r = getattr(oracle, case["solver"])(p["indptr"], p["indices"], p["data"], p["rhs"], x0, case["max_iter"], case["tol"],
                                        precond_diag=dg, trace_cap=case["max_iter"])
    o = getattr(kp, case["solver"])(p["indptr"], p["indices"], p["data"], p["rhs"], x0, case["max_iter"], case["tol"], prec=M)
    print("%s: oracle %d iterations, checker %d; rows agreeing at 1e-9: %d" % (case["name"], r.its, o.its, rows_close(r.trace, o.trace, 1e-9, 1e-12)))
    assert r.status == oracle.OK and o.status == kp.OK
    assert abs(o.its - r.its) <= max(5, r.its // 4)
    assert rows_close(r.trace, o.trace, 1e-9, 1e-12) >= 10
    assert np.max(np.abs(o.x - p["exact"])) < 1e-9 * max(1.0, np.max(np.abs(p["exact"])))


# ------------------------------------------------------------------------------------------------ 2. counts
@pytest.mark.parametrize("name,dt", [("cd24x20", dt) for dt in ALL] + [("cd64x64", F64), ("cg", F64), ("cg", C64)], ids=_ids)
def test_bicgstab_counts(name, dt):
    dtname = np.dtype(dt).name
    want = BICG_COUNTS[name][dtname]
    got = tuple(checker_run("bicgstab", name, dtname, k) for k in ("jacobi", "ilu", "amg"))
    print("bicgstab %s %s: Jacobi %d, ILU(0) %d, AMG %d iterations" % ((name, dtname) + tuple(o.its for o in got)))
    assert all(o.status == kp.OK for o in got) and tuple(o.its for o in got) == want
    assert all(2 * o.its <= max_iter_of("bicgstab", name, dtname, k) for o, k in zip(got, ("jacobi", "ilu", "amg")))
    if name == "cd24x20":
        assert got[1].its < got[0].its and got[2].its < got[0].its                # strictly fewer than Jacobi in all four types
        s = checker_run("bicgstab", name, dtname, "ilu_s3")
        assert (s.status, s.its) == (kp.OK, BICG_SWEEPS_COUNTS[dtname]) and got[1].its <= s.its < got[0].its
        none = checker_run("bicgstab", name, dtname, "none")
        assert none.status == kp.OK and none.its == got[0].its                    # (a constant diagonal: Jacobi only scales)


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_minres_counts(dt):
    dtname = np.dtype(dt).name
    got = tuple(checker_run("minres", "cg", dtname, k) for k in ("jacobi", "ilu", "amg"))
    print("minres cg %s: Jacobi %d, ILU(0) %d, AMG %d iterations" % ((dtname,) + tuple(o.its for o in got)))
    assert all(o.status == kp.OK for o in got) and tuple(o.its for o in got) == MINRES_COUNTS[dtname]
    assert got[1].its < got[0].its and got[2].its < got[0].its
    assert all(o.trace.shape == (o.its + 1, 8) for o in got)                       # `its` is 0-based: one row per iteration run


# ------------------------------------------------------------------------------------------------ 3. the trace prefix
BICG_GPU_CASES = [("cd24x20", dt, k) for dt in ALL for k in KINDS] + [("cd64x64", F64, "amg"), ("p3_12x11x10", F64, "ilu")]
MINRES_GPU_CASES = [("cg", dt, k) for dt in ALL for k in ("ilu", "amg")]


@pytest.mark.parametrize("solver,name,dt,kind", [("bicgstab",) + c for c in BICG_GPU_CASES] + [("minres",) + c for c in MINRES_GPU_CASES], ids=_ids)
def test_trace_prefix_of_the_gpu_cases(solver, name, dt, kind):
    """With its sums taken pairwise the checker keeps the status and the count within the GPU test's margin, and a prefix of at
    least one trace row (five in f64) within a tenth of the GPU tolerance."""
    dtname = np.dtype(dt).name
    a, b = checker_run(solver, name, dtname, kind), checker_run(solver, name, dtname, kind, "pairwise")
    k = trace_prefix(solver, name, dtname, kind)
    print("%s %s %s %s: %d iterations, %d trace rows, prefix %d" % (solver, name, dtname, kind, a.its, len(a.trace), k))
    assert a.status == b.status == kp.OK and abs(a.its - b.its) <= max(5, a.its // 4)
    if name == "p3_12x11x10":
        assert a.its == BICG_COUNTS[name][dtname][1]
    assert 1 <= k <= len(a.trace)
    if np.dtype(dt) == np.dtype(F64):
        assert k >= 5
    rtol, atol = gpu_tols(dt)
    assert rows_close(a.trace, b.trace, rtol, atol) >= k


# ------------------------------------------------------------------------------------------------ 4. MINRES' rule
@pytest.mark.parametrize("dt,kind", [(dt, k) for dt in (C64, C32) for k in ("ilu", "amg")], ids=_ids)
def test_minres_imaginary_part_stays_below_half_the_limit(dt, kind):
    """minres.rs:279-287 refuses M when im(b2) > eps re(b2), b2 = conj(v_new).M v_new.  A diagonal M makes im(b2) an exact zero; an
    applied one makes it rounding noise.  On the fixtures handed to the GPU test the ratio im / (eps re) stays below 0.5."""
    eps = np.finfo(np.float32 if is_single(dt) else np.float64).eps
    for sums in ("numpy", "pairwise"):
        o = checker_run("minres", "cg", np.dtype(dt).name, kind, sums)
        ratio = max(abs(im) / (eps * re) for _, re, im in o.events)
        print("minres cg %s %s %s: max |im b2| / (eps re b2) = %.3f over %d steps" % (np.dtype(dt).name, kind, sums, ratio, len(o.events)))
        assert o.status == kp.OK and all(re > 0 for _, re, _ in o.events)
        assert ratio < IMAG_RATIO_LIMIT


def test_minres_amg_on_an_indefinite_matrix_ends_in_invalid_preconditioner():
    ip, ix, d, rhs = system_of("indefinite", "float64")
    M = amg.Applier(hierarchy_of("indefinite", "float64"))
    for sums in ("numpy", "pairwise"):
        o = kp.minres(ip, ix, d, rhs, np.zeros(rhs.size), 50, 1e-10, prec=M, sums=sums)
        assert (o.status, o.its) == (kp.INVALID_PRECOND, INDEFINITE_MINRES[0])
        assert np.isclose(o.res, INDEFINITE_MINRES[1], rtol=1e-3)     # ten orders above the rounding of that sum


# ------------------------------------------------------------------------------------------------ 5. the restart branch
def test_restart_branch_under_an_applied_preconditioner():
    """One Jacobi sweep of ILU(0) (M = diag(U)^-1) leaves `restart_converges` on its way into the restart branch at iteration 1,
    in one copy and in 700; more sweeps and the AMG cycle (an exact LU of a 3 x 3 block) solve the system before rho can vanish,
    and `restart_then_w_zero_nan` has a zero pivot."""
    found = restart_cases()
    print("restart cases under an applied M:", found)
    assert ("restart_converges", 1, "ilu_s1", (1,), kp.OK, 4) in found
    assert ("restart_converges", 700, "ilu_s1", (1,), kp.OK, 4) in found
    assert all(kind == "ilu_s1" for _, _, kind, _, _, _ in found)


# ------------------------------------------------------------------------------------------------ 6. the C ABI
NEW_NAMES = sorted("sprs_%s_%s_solve%s_%s" % (pc, k, dev, s) for pc in ("ilu0", "amg") for k in ("bicgstab", "minres") for dev in ("", "_dev")
                   for s in "dzsc")


def test_the_32_entry_points_exist():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert len(NEW_NAMES) == 32
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sprsolve_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(sprs_[a-z0-9_]+)\s*\(", src))
    for name in NEW_NAMES:
        assert name in declared, name
        fn = getattr(L, name)                                  # AttributeError: the library does not export it
        assert fn.argtypes is not None and len(fn.argtypes) == 10, name
        assert fn(None, None, None, 4, None, 4, 10, 1e-8, None, None) == _lib.INVALID_ARGUMENT
    import sprsolve_amd
    with pytest.raises(TypeError):
        sprsolve_amd.CSMinRes.precond_solve(None, object(), None, None, 1, 1e-8)
