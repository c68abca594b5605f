"""The on-chip batch solvers on the GPU (sprs_batch_*, csrc/batch.hip) against the checker that restates their arithmetic with the
sums in the workgroup's order (tests/_batch_ref.py): the batched product and both solvers BIT FOR BIT in all four scalar types, the
events of the recurrences per system, many workgroups, the row caps, the refusals and the device entry points.

The systems, the tolerances and the checker's iteration counts are tests/test_batch_cpu.py's (which checks the checker on the CPU);
every max_iter is at least twice its count but for the system chosen to run out."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _batch_ref as ref  # noqa: E402
from test_batch_cpu import (ALL, C64, F64, MAX_ITER, NBATCH, SHAPES, SOLVERS, SPECIAL_MAX_ITER, SPECIAL_TOL, checked, special, system,  # noqa: E402
                            tol_of)
from test_gpu_ilu import _margin  # noqa: E402

pytestmark = pytest.mark.gpu

_ids = lambda v: v if isinstance(v, str) else np.dtype(v).name


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def _n(shape):
    return shape[0] * shape[1]


# ------------------------------------------------------------------------------------------------ 1. the product, bit for bit
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_product_bits(sa, dt):
    for shape in SHAPES:
        ip, ix, V, RHS = system(shape, dt, "bicgstab")
        n = _n(shape)
        B = sa.BatchCsr.new(n, ip, ix, V)
        info = B.info
        assert (info["n"], info["nnz"], info["nbatch"], info["threads"]) == (n, ix.size, NBATCH, ref.threads(n))
        assert info["lds_cg"] == ref.lds_bytes("cg", dt, n) and info["lds_bicgstab"] == ref.lds_bytes("bicgstab", dt, n)
        assert same_bits(B.values(), np.array(V))
        X = np.array(RHS)                                     # any vectors: the right-hand sides
        Y = np.full_like(X, 7)
        B.mul_vec(X, Y)
        assert same_bits(Y, ref.mul_vec(ip, ix, V, X)), shape
        V2 = np.ascontiguousarray((V[::-1] * 1.5).astype(dt))  # other values on the same pattern and plan
        B.set_values(V2)
        assert same_bits(B.values(), V2)
        B.mul_vec(X, Y)
        assert same_bits(Y, ref.mul_vec(ip, ix, V2, X)), shape
        B.close()


# ------------------------------------------------------------------------------------------------ 2. the solves, bit for bit
@pytest.mark.parametrize("jacobi", [False, True], ids=["none", "jacobi"])
@pytest.mark.parametrize("dt", ALL, ids=_ids)
@pytest.mark.parametrize("solver", SOLVERS)
def test_solve_bits(sa, solver, dt, jacobi):
    for shape in SHAPES:
        ip, ix, V, RHS = system(shape, dt, solver)
        n = _n(shape)
        B = sa.BatchCsr.new(n, ip, ix, V)
        X = np.zeros_like(RHS)
        its, res, status = getattr(B, solver)(RHS, X, MAX_ITER, tol_of(dt), precond="jacobi" if jacobi else None)
        wx, wits, wres, wstatus, wret = checked(solver, shape, dt, jacobi)
        print(solver, np.dtype(dt).name, jacobi, shape, "its", its.tolist(), "checker", wits.tolist(), "max|x - checker|", np.max(np.abs(X - wx)))
        assert B.last_status == wret == 0
        assert np.array_equal(status, wstatus) and np.array_equal(its, wits), shape
        assert same_bits(res, wres), shape
        assert same_bits(X, np.array(wx)), shape              # the whole (nbatch, n) block: nobody writes into a neighbour's rows
        B.close()


# ------------------------------------------------------------------------------------------------ 3. every system stops on its own
@pytest.mark.parametrize("solver", SOLVERS)
def test_every_system_stops_on_its_own(sa, solver):
    ip, ix, V, RHS, X0, (wx, wits, wres, wstatus, wret) = special(solver)
    B = sa.BatchCsr.new(ip.size - 1, ip, ix, V)
    X = np.array(X0)
    its, res, status = getattr(B, solver)(RHS, X, SPECIAL_MAX_ITER[solver], SPECIAL_TOL)
    print(solver, "status", status.tolist(), "its", its.tolist())
    assert status.tolist() == wstatus.tolist() and its.tolist() == wits.tolist()
    assert sorted(set(status.tolist())) == [ref.OK, ref.INSUFFICIENT_ITER, ref.BREAKDOWN]
    assert same_bits(res, wres) and same_bits(X, np.array(wx))
    assert B.last_status == wret == ref.INSUFFICIENT_ITER     # the lowest-numbered system that did not return Ok
    assert not np.any(X[1]) and its[1] == 0 and its[2] == 0 and same_bits(X[2], np.array(X0[2]))
    B.close()


# ------------------------------------------------------------------------------------------------ 4. many workgroups
def test_many_workgroups(sa):
    from sprsolve_amd import gen
    NB, tol = 3000, 1e-8
    ip, ix, V, RHS = gen.batch_convection_diffusion(6, 5, NB, F64)
    n = 30
    B = sa.BatchCsr.new(n, ip, ix, V)
    X = np.zeros_like(RHS)
    its, res, status = B.bicgstab(RHS, X, MAX_ITER, tol, precond="jacobi")
    assert B.last_status == 0 and not np.any(status) and 2 * its.max() <= MAX_ITER
    assert len(set(its.tolist())) > 3                         # visibly different iteration counts
    for b in (0, 1499, 2999):
        o = ref.bicgstab(ip, ix, V[b], RHS[b], np.zeros(n), MAX_ITER, tol, jacobi=True)
        assert (o.status, o.its) == (status[b], its[b]) and same_bits(X[b], o.x) and res[b] == o.res, b
    # the true residual of every system, on the host
    AX = np.add.reduceat(V * X[:, ix], ip[:-1], axis=1)
    true = np.linalg.norm(RHS - AX, axis=1) / np.linalg.norm(RHS, axis=1)
    bound = tol * np.array([_margin(int(i)) for i in its])    # tol times the margin tests/test_gpu_ilu.py uses
    print("its", its.min(), its.max(), "worst true residual / tol", (true / tol).max())
    assert np.all(true < bound)
    # a second call gives the same bytes
    X2 = np.zeros_like(RHS)
    its2, res2, status2 = B.bicgstab(RHS, X2, MAX_ITER, tol, precond="jacobi")
    assert same_bits(X2, X) and np.array_equal(its2, its) and same_bits(res2, res) and np.array_equal(status2, status)
    B.close()
    # the same system in a batch of 1 gives the bytes it gave in the batch of 3000
    for b in (0, 1499, 2999):
        B1 = sa.BatchCsr.new(n, ip, ix, V[b:b + 1])
        x1 = np.zeros((1, n))
        i1, r1, s1 = B1.bicgstab(RHS[b:b + 1], x1, MAX_ITER, tol, precond="jacobi")
        assert same_bits(x1[0], X[b]) and i1[0] == its[b] and r1[0] == res[b] and s1[0] == 0
        B1.close()


# ------------------------------------------------------------------------------------------------ 5. the cap
def _tridiagonal(n, nbatch, dt):
    from sprsolve_amd import gen
    ip = np.zeros(n + 1, np.int32)
    ip[1:] = np.cumsum(np.where((np.arange(n) == 0) | (np.arange(n) == n - 1), 2, 3))
    ix = np.concatenate([[c for c in (i - 1, i, i + 1) if 0 <= c < n] for i in range(n)]).astype(np.int32)
    rows = np.repeat(np.arange(n), np.diff(ip))
    V = np.zeros((nbatch, ix.size), dt)
    for b in range(nbatch):
        c = 0.2 + 0.1 * b
        V[b] = np.where(ix == rows, 2.5 + 0.5 * b, np.where(ix < rows, -1.0 - c, -1.0 + c))
    X = (1.0 + gen.uniform(gen.SEED, nbatch * n, stream=440).reshape(nbatch, n)).astype(dt)
    return ip, ix, V, ref.mul_vec(ip, ix, V, X)


def test_row_cap(sa):
    cap = sa.BatchCsr.max_rows("bicgstab", F64)
    assert cap == ref.max_rows("bicgstab", F64) == 1024
    tol = 1e-8
    ip, ix, V, RHS = _tridiagonal(cap, 2, F64)
    B = sa.BatchCsr.new(cap, ip, ix, V)
    assert B.info["lds_bicgstab"] == 128 + 8 * 8 * cap
    X = np.zeros_like(RHS)
    its, res, status = B.bicgstab(RHS, X, 200, tol)           # (the checker: 18 and 14 iterations)
    assert not np.any(status) and 2 * its.max() <= 200
    true = np.linalg.norm(RHS - np.add.reduceat(V * X[:, ix], ip[:-1], axis=1), axis=1) / np.linalg.norm(RHS, axis=1)
    print("at the cap: its", its.tolist(), "true residual / tol", (true / tol).tolist())
    assert np.all(true < tol * np.array([_margin(int(i)) for i in its]))
    o = ref.bicgstab(ip, ix, V[1], RHS[1], np.zeros(cap), 200, tol)
    assert (o.status, o.its) == (0, its[1]) and same_bits(X[1], o.x)
    B.close()
    # one row more: refused, with n and the cap in the text; nothing is truncated and nothing falls back
    ip, ix, V, RHS = _tridiagonal(cap + 1, 1, F64)
    B = sa.BatchCsr.new(cap + 1, ip, ix, V)
    X = np.zeros_like(RHS)
    with pytest.raises(ValueError, match=r"%d.*%d" % (cap + 1, cap)):
        B.bicgstab(RHS, X, 200, tol)
    assert not np.any(X)
    # ... while cg takes that size (its cap is 1600) — the matrix made symmetric positive definite
    assert sa.BatchCsr.max_rows("cg", F64) == 1600
    rows = np.repeat(np.arange(cap + 1), np.diff(ip))
    Vs = np.where(ix == rows, 2.5, -1.0)[None, :].copy()
    B.set_values(Vs)
    rhs = ref.mul_vec(ip, ix, Vs, np.ones((1, cap + 1)))
    its, res, status = B.cg(rhs, X, 200, tol)
    assert status[0] == 0 and 2 * its[0] <= 200 and np.max(np.abs(X - 1.0)) < 1e-6
    B.close()
    # c64 is refused at a size at which f64 is taken
    ipc, ixc, Vc, RHSc = _tridiagonal(cap, 1, C64)
    Bc = sa.BatchCsr.new(cap, ipc, ixc, Vc)
    with pytest.raises(ValueError, match=r"%d.*%d" % (cap, sa.BatchCsr.max_rows("bicgstab", C64))):
        Bc.bicgstab(RHSc, np.zeros_like(RHSc), 200, tol)
    Bc.close()


# ------------------------------------------------------------------------------------------------ 6. the refusals
def test_errors(sa):
    from sprsolve_amd import _lib
    E = sa.error
    L = _lib.lib()
    ip, ix, V, RHS = system((6, 5), F64, "bicgstab")
    n = 30
    # unsorted columns at creation: the row is named
    bad = np.array(ix)
    a, b = ip[7], ip[7] + 1
    bad[a], bad[b] = bad[b], bad[a]
    with pytest.raises(ValueError, match="row 7 "):
        sa.BatchCsr.new(n, ip, bad, V)
    dup = np.array(ix); dup[ip[3] + 1] = dup[ip[3]]
    with pytest.raises(ValueError, match="row 3 "):
        sa.BatchCsr.new(n, ip, dup, V)
    h = C.c_void_p(); row = C.c_int64(-2)
    ctx = sa.default_ctx(0)
    vp = lambda arr: arr.ctypes.data_as(C.c_void_p)
    Vc = np.ascontiguousarray(V)
    assert L.sprs_batch_create_d(ctx.h, n, ix.size, NBATCH, vp(ip), vp(bad), vp(Vc), C.byref(h), C.byref(row)) == 7 and row.value == 7 and not h.value
    assert L.sprs_batch_create_d(ctx.h, n, ix.size, -1, vp(ip), vp(ix), vp(Vc), C.byref(h), None) == 7
    assert L.sprs_batch_create_d(ctx.h, -1, ix.size, NBATCH, vp(ip), vp(ix), vp(Vc), C.byref(h), None) == 7
    assert L.sprs_batch_create_d(ctx.h, n, ix.size, NBATCH, None, vp(ix), vp(Vc), C.byref(h), None) == 7 and not h.value
    # wrong lengths
    B = sa.BatchCsr.new(n, ip, ix, V)
    X = np.zeros_like(RHS)
    for solve in (B.bicgstab, B.cg):
        with pytest.raises(E.IncompatibleMatrixFormat, match="Input vec dimension"):
            solve(RHS[:4], X, 10, 1e-8)
        with pytest.raises(E.IncompatibleMatrixFormat, match="output vec dimension"):
            solve(RHS, np.zeros((NBATCH, n - 1)), 10, 1e-8)
    with pytest.raises(E.DimensionMismatch):
        B.mul_vec(RHS[:4], np.zeros((4, n)))
    with pytest.raises(ValueError):
        B.bicgstab(RHS, X, 10, 1e-8, precond="ilu")
    assert L.sprs_batch_bicgstab_solve_d(B.h, 2, vp(np.array(RHS)), RHS.size, vp(X), X.size, 10, 1e-8, None, None, None) == 7
    assert L.sprs_batch_bicgstab_solve_z(B.h, 0, vp(np.array(RHS)), RHS.size, vp(X), X.size, 10, 1e-8, None, None, None) == 7      # another scalar type
    assert not np.any(X)
    B.close()
    # Jacobi on a pattern without a full diagonal: ZeorDiagonalElem with the smallest such row, for the whole call
    rows = np.repeat(np.arange(n), np.diff(ip))
    keep = ~((rows == ix) & ((rows == 11) | (rows == 20)))
    ip2 = np.zeros(n + 1, np.int32); ip2[1:] = np.cumsum(np.bincount(rows[keep], minlength=n))
    B = sa.BatchCsr.new(n, ip2, ix[keep], np.ascontiguousarray(V[:, keep]))
    for solve in (B.bicgstab, B.cg):
        with pytest.raises(E.ZeorDiagonalElem) as ei:
            solve(RHS, X, 10, 1e-8, precond="jacobi")
        assert ei.value.row == 11 and not np.any(X)
    its, res, status = B.bicgstab(RHS, X, 3, 1e-8)            # ... and only an error when Jacobi is asked for
    assert status.tolist() == [3] * NBATCH and np.any(X)
    B.close()
    # a NULL handle
    assert L.sprs_batch_destroy(None) == 0
    assert L.sprs_batch_info(None, None, None, None, None, None, None) == 7
    assert L.sprs_batch_mul_vec_d(None, None, 0, None, 0) == 7 and L.sprs_batch_cg_solve_d(None, 0, None, 0, None, 0, 1, 1e-8, None, None, None) == 7
    # nbatch = 0 and n = 0: every call returns 0 and touches nothing
    for nn, nb in ((n, 0), (0, 3)):
        ipe, ixe = (ip, ix) if nn else (np.zeros(1, np.int32), np.zeros(0, np.int32))
        B = sa.BatchCsr.new(nn, ipe, ixe, np.zeros((nb, ixe.size)))
        assert (B.info["n"], B.info["nbatch"], B.info["threads"]) == (nn, nb, ref.threads(nn))
        e = np.zeros((nb, nn))
        B.mul_vec(e, e.copy()); B.set_values(np.zeros((nb, ixe.size)))
        assert B.values().shape == (nb, ixe.size)
        guard_i = (C.c_size_t * 4)(9, 9, 9, 9); guard_r = (C.c_double * 4)(9, 9, 9, 9); guard_s = (C.c_int * 4)(9, 9, 9, 9)
        for name in ("sprs_batch_bicgstab_solve_d", "sprs_batch_cg_solve_d"):
            for pc in (0, 1):
                assert getattr(L, name)(B.h, pc, None, 0, None, 0, 10, 1e-8, guard_i, guard_r, guard_s) == 0
        assert list(guard_i) == [9] * 4 and list(guard_r) == [9.0] * 4 and list(guard_s) == [9] * 4
        its, res, status = B.cg(e, e.copy(), 10, 1e-8)
        assert its.shape == res.shape == status.shape == (nb,) and B.last_status == 0
        B.close()


# ------------------------------------------------------------------------------------------------ 7. the device entry points
@pytest.mark.parametrize("dt", [F64, C64], ids=_ids)
def test_device_entry_points(sa, dt):
    import torch
    shape = (13, 5)
    for solver in SOLVERS:
        ip, ix, V, RHS = system(shape, dt, solver)
        n = _n(shape)
        dV = sa.DevVec.from_numpy(np.array(V).ravel())
        Bd = sa.BatchCsr.new(n, torch.from_numpy(np.array(ip)).cuda(), torch.from_numpy(np.array(ix)).cuda(), dV)        # create_dev: all on the device
        Bh = sa.BatchCsr.new(n, ip, ix, dV)                                                                             # ... the pattern uploaded by the mirror
        assert (Bd.nbatch, Bd.nnz) == (Bh.nbatch, Bh.nnz) == (NBATCH, ix.size)
        assert same_bits(Bd.values(), np.array(V)) and same_bits(Bh.values(), np.array(V))
        dX = sa.DevVec.from_numpy(np.array(RHS).ravel()); dY = sa.DevVec(NBATCH * n, dt)
        Bd.mul_vec(dX, dY)
        assert same_bits(dY.to_numpy().reshape(NBATCH, n), ref.mul_vec(ip, ix, V, RHS))
        for jacobi in (False, True):
            wx, wits, wres, wstatus, _ = checked(solver, shape, dt, jacobi)
            dR = sa.DevVec.from_numpy(np.array(RHS).ravel()); dS = sa.DevVec(NBATCH * n, dt); dS.zero()
            its, res, status = getattr(Bd, solver)(dR, dS, MAX_ITER, tol_of(dt), precond="jacobi" if jacobi else None)
            assert np.array_equal(its, wits) and same_bits(res, wres) and np.array_equal(status, wstatus)
            assert same_bits(dS.to_numpy().reshape(NBATCH, n), np.array(wx))
        V2 = np.ascontiguousarray((V * 0.5).astype(dt))
        Bd.set_values(sa.DevVec.from_numpy(V2.ravel()))
        assert same_bits(Bd.values(), V2)
        with pytest.raises(TypeError):
            Bd.bicgstab(dR, np.zeros((NBATCH, n), dt), 10, 1e-8)
        Bd.close(); Bh.close()
