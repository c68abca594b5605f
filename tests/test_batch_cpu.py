"""The on-chip batch solvers without a GPU: the C ABI and the Python mirror exist and refuse what they must; the plan as the
library states it equals the checker's independent restatement; and the checker of the GPU tests (tests/_batch_ref.py, sums in the
workgroup's order) follows the recurrences it restates — its BiCGStab against the CPU oracle (serial sums), its CG against
tests/_cg_ref.py (numpy's sums) — on every system tests/test_gpu_batch.py uses, with the statuses the special systems were chosen
for.  The systems, the tolerances and the checker's iteration counts are defined here and imported by the GPU tests.

Tolerances: nothing is invented.  Iteration counts may differ by tests/test_gpu_cg.py's `_margin` (what a changed summation order
is allowed there and in __graft_entry__.smoke); x by what tests/test_gpu_cg.py::test_fused_follows_literal allows two summation
orders of one recurrence: 1e-7 max|x| (f64, c64), 2e-3 (f32) and 5e-3 (c32) absolute; tol is tests/test_ilu_cpu.py's tol_of."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _batch_ref as ref  # noqa: E402
import _cg_ref  # noqa: E402
from test_gpu_cg import _margin  # noqa: E402
from test_ilu_cpu import ALL, C64, F64, is_single, tol_of  # noqa: E402

_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name

SHAPES = [(6, 5), (8, 8), (13, 5), (20, 15)]      # n = 30: a partial wavefront; 64: exactly one; 65: two, the second nearly empty;
NBATCH = 5                                        # 300: B = 256, threads take two rows
SOLVERS = ("bicgstab", "cg")

# The checker's largest iteration count over the five systems of every shape, x0 = 0, tol = tol_of(dtype), in the order of SHAPES,
# keyed by (solver, dtype, Jacobi).  MAX_ITER is at least twice the largest.
COUNTS = {
    ("bicgstab", "float64", False): (13, 15, 17, 25), ("bicgstab", "float64", True): (13, 14, 18, 25),
    ("bicgstab", "complex128", False): (13, 15, 19, 25), ("bicgstab", "complex128", True): (13, 15, 18, 25),
    ("bicgstab", "float32", False): (9, 11, 13, 18), ("bicgstab", "float32", True): (9, 11, 13, 17),
    ("bicgstab", "complex64", False): (9, 11, 13, 16), ("bicgstab", "complex64", True): (8, 11, 12, 17),
    ("cg", "float64", False): (21, 26, 26, 34), ("cg", "float64", True): (20, 25, 26, 33),
    ("cg", "complex128", False): (21, 27, 27, 34), ("cg", "complex128", True): (21, 26, 26, 33),
    ("cg", "float32", False): (13, 14, 15, 18), ("cg", "float32", True): (12, 14, 14, 17),
    ("cg", "complex64", False): (13, 15, 15, 18), ("cg", "complex64", True): (13, 14, 15, 17),
}
MAX_ITER = 80


def x_close(x, want, dt):
    if is_single(dt):
        return np.max(np.abs(x - want)) < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
    return np.max(np.abs(x - want)) <= 1e-7 * max(1.0, np.max(np.abs(want)))


@functools.lru_cache(maxsize=None)
def _system_cached(shape, dtname, hermitian):
    from sprsolve_amd import gen
    dt = np.dtype(dtname)
    ip, ix, V, _ = gen.batch_convection_diffusion(shape[0], shape[1], NBATCH, dt, hermitian=hermitian)
    n = ip.size - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    dg = rows == ix
    V = V.copy()
    for b in range(NBATCH):                       # a diagonal that varies along the rows: Jacobi is no constant scaling
        V[b, dg] = (V[b, dg] * (1.25 + 0.25 * gen.uniform(gen.SEED, n, stream=410 + b))).astype(dt)
    x = (1.0 + gen.uniform(gen.SEED, NBATCH * n, stream=420).reshape(NBATCH, n)).astype(dt)
    if dt.kind == "c":
        x = (x + 1j * gen.uniform(gen.SEED, NBATCH * n, stream=421).reshape(NBATCH, n)).astype(dt)
    RHS = ref.mul_vec(ip, ix, V, x)
    for a in (ip, ix, V, RHS):
        a.setflags(write=False)
    return ip, ix, V, RHS


def system(shape, dt, solver):
    """(indptr, indices, values (5, nnz), rhs (5, n)) of a shape for a solver (CG: the Hermitian positive-definite variant): the
    generator's batch with every diagonal entry scaled by a factor in [1, 1.5) of its own, rhs_b = A_b x_b for a uniform x_b.
    Read-only and shared."""
    return _system_cached(tuple(shape), np.dtype(dt).name, solver == "cg")


@functools.lru_cache(maxsize=None)
def _checked_cached(solver, shape, dtname, jacobi):
    dt = np.dtype(dtname)
    ip, ix, V, RHS = system(shape, dt, solver)
    out = ref.solve_batch(solver, ip, ix, V, RHS, np.zeros_like(RHS), MAX_ITER, tol_of(dt), jacobi)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def checked(solver, shape, dt, jacobi):
    """The checker's (X, its, res, status, return value) of a whole batch from x0 = 0: computed once, shared, read-only."""
    return _checked_cached(solver, tuple(shape), np.dtype(dt).name, bool(jacobi))


def diag_of(ip, ix, v):
    n = ip.size - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    return v[rows == ix]


# ---- the special systems on the 6 x 5 pattern, f64, x0 = 0 unless said: (values (5, nnz), rhs, x0, max_iter, what to expect)
SPECIAL_MAX_ITER = {"bicgstab": 40, "cg": 44}                 # >= 2 * 13 and >= 2 * 21, the 6 x 5 counts; the fourth system runs out
SPECIAL_TOL = 1e-10
SPECIAL_EXPECT = {                                            # (status, its) per system, from the checker
    "bicgstab": [(ref.OK, 11), (ref.OK, 0), (ref.OK, 0), (ref.INSUFFICIENT_ITER, 40), (ref.BREAKDOWN, 3)],
    "cg": [(ref.OK, 17), (ref.OK, 0), (ref.OK, 0), (ref.INSUFFICIENT_ITER, 44), (ref.BREAKDOWN, 1)],
}


@functools.lru_cache(maxsize=None)
def special(solver):
    """One batch of five on the 6 x 5 pattern: an ordinary system; one with rhs = 0 (x0 = 1: the answer is x = 0 after 0
    iterations); one whose x0 already solves it; one that runs out of max_iter; one that ends in BreakDown.
    BiCGStab.  Runs out: system 1 with every diagonal entry set to 1 (indefinite).  BreakDown: the identity but for the block
    [[2, 3], [2, 2]] on unknowns 0 and 1, rhs = (1, 2, 0, ..): conj(r0).v is exactly zero in the loop's third pass (found by running
    the checker over small integer blocks; the plain rotation [[0, 1], [-1, 0]] does NOT end so: conj(r0).v = 0 in the unchecked
    first step makes everything NaN and the solve runs to max_iter).
    CG.  Runs out: system 1 scaled as S A S with S = diag(10^(2 i / (n - 1))).  BreakDown: system 1 with every diagonal entry set to
    2.5 (indefinite): re(conj(p).q) <= 0 in the second pass."""
    ip, ix, V0, R0 = system((6, 5), F64, solver)
    n = ip.size - 1
    rows = np.repeat(np.arange(n), np.diff(ip))
    dg = rows == ix
    V = np.array(V0); RHS = np.array(R0); X0 = np.zeros_like(RHS)
    RHS[1] = 0.0; X0[1] = 1.0
    X0[2] = np.linalg.solve(_cg_ref.dense(ip, ix, V[2]), RHS[2])
    V[3] = V0[1]; RHS[3] = R0[1]
    V[4] = V0[1]; RHS[4] = R0[1]
    if solver == "bicgstab":
        V[3, dg] = 1.0
        V[4] = 0.0; V[4, dg] = 1.0
        for (r, c), a in {(0, 0): 2.0, (0, 1): 3.0, (1, 0): 2.0, (1, 1): 2.0}.items():
            V[4, np.nonzero((rows == r) & (ix == c))[0][0]] = a
        RHS[4] = 0.0; RHS[4, 0] = 1.0; RHS[4, 1] = 2.0
    else:
        s = 10.0 ** (2.0 * np.arange(n) / (n - 1.0))
        V[3] = V0[1] * s[rows] * s[ix]
        V[4, dg] = 2.5
    out = ref.solve_batch(solver, ip, ix, V, RHS, X0, SPECIAL_MAX_ITER[solver], SPECIAL_TOL)
    for a in (V, RHS, X0) + out[:4]:
        a.setflags(write=False)
    return ip, ix, V, RHS, X0, out


# ------------------------------------------------------------------------------------------------ the ABI and the plan
@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


NAMES = sorted(["sprs_batch_%s_%s" % (f, s) for f in ("create", "create_dev", "set_values", "set_values_dev", "read", "mul_vec", "mul_vec_dev",
                                                      "bicgstab_solve", "bicgstab_solve_dev", "cg_solve", "cg_solve_dev") for s in "dzsc"]
               + ["sprs_batch_destroy", "sprs_batch_info", "sprs_batch_max_rows"])


def test_batch_abi_and_binding_exist(L):
    src = open(os.path.join(ROOT, "include", "sprsolve_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(n for n in set(re.findall(r"\b(sprs_[a-z0-9_]+)\s*\(", src)) if n.startswith("sprs_batch_"))
    assert declared == NAMES
    assert re.search(r"typedef\s+struct\s+sprs_batch\s+sprs_batch\s*;", src)
    for name in NAMES:
        assert hasattr(L, name), name
    out = C.c_void_p(); row = C.c_int64(0)
    for s in "dzsc":
        assert getattr(L, "sprs_batch_create_" + s)(None, 4, 0, 1, None, None, None, C.byref(out), C.byref(row)) == 7 and not out.value
        assert getattr(L, "sprs_batch_create_dev_" + s)(None, 4, 0, 1, None, None, None, C.byref(out), C.byref(row)) == 7 and not out.value
        assert getattr(L, "sprs_batch_set_values_" + s)(None, None) == 7 and getattr(L, "sprs_batch_read_" + s)(None, None) == 7
        assert getattr(L, "sprs_batch_mul_vec_dev_" + s)(None, None, 0, None, 0) == 7
        for k in ("bicgstab_solve", "bicgstab_solve_dev", "cg_solve", "cg_solve_dev"):
            assert getattr(L, "sprs_batch_%s_%s" % (k, s))(None, 0, None, 0, None, 0, 10, 1e-8, None, None, None) == 7
    assert L.sprs_batch_destroy(None) == 0 and L.sprs_batch_info(None, None, None, None, None, None, None) == 7
    import sprsolve_amd
    assert callable(sprsolve_amd.BatchCsr.new) and callable(sprsolve_amd.BatchCsr.bicgstab) and callable(sprsolve_amd.BatchCsr.cg)


def test_caps_of_the_library_are_the_checkers(L):
    import sprsolve_amd as sa
    for code, solver in enumerate(SOLVERS):
        for dcode, dt in enumerate(ALL):                      # the handles' dtype codes follow ALL: f64, c64, f32, c32
            assert L.sprs_batch_max_rows(code, dcode) == ref.max_rows(solver, dt) == sa.BatchCsr.max_rows(solver, dt)
    assert ref.max_rows("bicgstab", F64) == 1024 and ref.max_rows("bicgstab", C64) == 512          # the two the header quotes
    assert L.sprs_batch_max_rows(2, 0) == -1 and L.sprs_batch_max_rows(0, 4) == -1
    assert [ref.threads(n) for n in (0, 1, 64, 65, 128, 129, 256, 257, 1024)] == [64, 64, 64, 128, 128, 192, 256, 256, 256]


def test_generator():
    from sprsolve_amd import gen
    for dt in ALL:
        ip, ix, V, RHS = gen.batch_convection_diffusion(6, 5, 4, dt)
        n = 30
        assert V.shape == (4, ip[-1]) and RHS.shape == (4, n) and V.dtype == RHS.dtype == np.dtype(dt) and ip.dtype == ix.dtype == np.int32
        ip1, ix1, d1, _ = gen.convection_diffusion_2d(6, 5)
        assert np.array_equal(ip, ip1) and np.array_equal(ix, ix1)
        assert len({V[b].tobytes() for b in range(4)}) == 4                                  # values of their own
        assert np.array_equal(RHS, ref.mul_vec(ip, ix, V, np.broadcast_to(
            ((1.0 + (np.arange(n) // 5 + 2.0 * (np.arange(n) % 5)) / 11.0) * ((1.0 - 0.5j) if np.dtype(dt).kind == "c" else 1.0)).astype(dt), (4, n))))
        ip, ix, V, RHS = gen.batch_convection_diffusion(6, 5, 4, dt, hermitian=True)
        for b in range(4):
            M = _cg_ref.dense(ip, ix, V[b]).astype(np.complex128)
            assert np.array_equal(M, M.conj().T) and np.linalg.eigvalsh(M).min() > 0
        if np.dtype(dt).kind == "c":
            assert np.any(V.imag != 0)
    ip, ix, V, RHS = gen.batch_convection_diffusion(6, 5, 0, F64)
    assert V.shape == (0, ip[-1]) and RHS.shape == (0, 30)


# ------------------------------------------------------------------------------------------------ the checker follows its recurrences
@pytest.mark.parametrize("jacobi", [False, True], ids=["none", "jacobi"])
@pytest.mark.parametrize("dt", ALL, ids=_ids)
@pytest.mark.parametrize("solver", SOLVERS)
def test_checker_follows_the_recurrence(oracle, solver, dt, jacobi):
    tol = tol_of(dt)
    worst = []
    for shape in SHAPES:
        ip, ix, V, RHS = system(shape, dt, solver)
        n = ip.size - 1
        X, its, res, status, ret = checked(solver, shape, dt, jacobi)
        assert ret == ref.OK and not np.any(status)
        for b in range(NBATCH):
            dg = diag_of(ip, ix, V[b]) if jacobi else None    # V = T: the diagonal in the scalar type
            if solver == "bicgstab":
                o = oracle.bicgstab(ip, ix, V[b], RHS[b], np.zeros(n, dt), MAX_ITER, tol, precond_diag=dg)
            else:
                o = _cg_ref.cg(ip, ix, V[b], RHS[b], np.zeros(n, dt), MAX_ITER, tol, precond_diag=dg)
            assert o.status == ref.OK
            assert abs(int(its[b]) - o.its) <= _margin(o.its), (shape, b, its[b], o.its)
            assert x_close(X[b], o.x, dt), (shape, b)
            assert res[b] <= tol and res.dtype == (np.float32 if is_single(dt) else np.float64)
        worst.append(int(its.max()))
        assert len(set(its.tolist())) > 1                     # the systems need visibly different iteration counts
    print(solver, np.dtype(dt).name, jacobi, worst)
    assert tuple(worst) == COUNTS[(solver, np.dtype(dt).name, jacobi)]
    assert 2 * max(worst) <= MAX_ITER


@pytest.mark.parametrize("solver", SOLVERS)
def test_special_systems_end_as_chosen(oracle, solver):
    ip, ix, V, RHS, X0, (X, its, res, status, ret) = special(solver)
    n = ip.size - 1
    got = list(zip(status.tolist(), its.tolist()))
    assert got == SPECIAL_EXPECT[solver], got
    assert ret == ref.INSUFFICIENT_ITER                       # the lowest-numbered system that did not return Ok
    assert np.all(np.isfinite(X))                             # (NaN payloads would not compare bit for bit)
    assert not np.any(X[1]) and res[1] == 0.0 and np.array_equal(X[2], X0[2])
    assert 2 * its[0] <= SPECIAL_MAX_ITER[solver]
    for b in range(NBATCH):                                   # the same events from the recurrence's other restatement
        if solver == "bicgstab":
            o = oracle.bicgstab(ip, ix, V[b], RHS[b], X0[b], SPECIAL_MAX_ITER[solver], SPECIAL_TOL)
        else:
            o = _cg_ref.cg(ip, ix, V[b], RHS[b], X0[b], SPECIAL_MAX_ITER[solver], SPECIAL_TOL)
        assert o.status == status[b] and abs(o.its - its[b]) <= (_margin(o.its) if o.status == ref.OK else 0), (b, o.status, o.its)
    if solver == "bicgstab":                                  # the rotation the docstring warns about
        v = np.zeros(ip[-1]); rows = np.repeat(np.arange(n), np.diff(ip)); v[rows == ix] = 1.0
        v[np.nonzero((rows == 0) & (ix == 0))[0][0]] = 0.0; v[np.nonzero((rows == 1) & (ix == 1))[0][0]] = 0.0
        v[np.nonzero((rows == 0) & (ix == 1))[0][0]] = 1.0; v[np.nonzero((rows == 1) & (ix == 0))[0][0]] = -1.0
        b = np.zeros(n); b[0] = 1.0
        o = ref.bicgstab(ip, ix, v, b, np.zeros(n), 12, 1e-10)
        assert (o.status, o.its) == (ref.INSUFFICIENT_ITER, 12)


def test_checker_sums_in_the_workgroup_order(oracle):
    """B = 256: the checker's sums are the oracle's emulation of the library's block_sum order with one workgroup."""
    from sprsolve_amd import gen
    for n in (30, 64, 65, 300, 700):
        for dt in (F64, C64):
            a = gen.uniform(gen.SEED, n, stream=430).astype(dt); b = gen.uniform(gen.SEED, n, stream=431).astype(dt)
            if np.dtype(dt).kind == "c":
                a = a + 1j * gen.uniform(gen.SEED, n, stream=432); b = b - 1j * gen.uniform(gen.SEED, n, stream=433)
            ip = np.arange(n + 1, dtype=np.int32); ix = np.arange(n, dtype=np.int32)
            A = ref._Sys(ip, ix, np.ones(n, dt), nthreads=256)
            d = A.cdot(A.vec(a), A.vec(b))
            mine = complex(d[0], d[1]) if A.S.cx else float(d)
            if np.dtype(dt) == np.dtype(F64):                 # (the oracle's emulation walks 16-byte packs: elementwise for c64, pairs for f64)
                continue
            oracle.set_reduction_order("gpu", grid=1)
            try:
                want = oracle.conj_dot_gpu_order(a, b)
                wn = oracle.norm2_gpu_order(a)
            finally:
                oracle.set_reduction_order("reference")
            assert mine == complex(want) and float(A.norm2(A.vec(a))) == float(wn)
