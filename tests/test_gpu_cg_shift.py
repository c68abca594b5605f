"""Multi-shift conjugate gradients (sprs_cgshift_*, csrc/cg_shift_fuse.hpp) against the checker (tests/_cg_shift_ref.py): every
dtype, the independence of a column from its neighbours and from `poll`, frozen columns and the events of the recurrence, the
shapes where the kernels take another path, the arguments and the entry points.

The checker's iteration counts (f64 / c64 at tol 1e-10, f32 / c32 at 1e-5), computed on the CPU:
    gen.symmetric_banded(2000) / gen.hermitian_banded(1500, 3), shifts 0, 1/32, 1/4, 1, 4, 16, 64, 1024:
        f64 26 26 25 22 16 10 7 4    c64 26 26 24 21 16 10 7 4    f32 14 14 13 11 8 5 4 2    c32 13 13 12 11 8 5 4 2
    gen.poisson3d(13, 11, 9) (1287 rows), shifts 0, 1/4, 1, 16, 1024:    f64 45 40 31 11 4    c32 28 24 17 6 2
    the 3 x 3 matrix, the eight shifts: 3 for every shift (f32 / c32: 2 for sigma = 1024)
MAX_ITER = 80 is at least three times the largest count of the banded systems."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cg_ref as ref  # noqa: E402
import _cg_shift_ref as shift  # noqa: E402

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
MAX_ITER = 80
SHIFTS = [0.0, 1.0 / 32, 0.25, 1.0, 4.0, 16.0, 64.0, 1024.0]
SHIFTS3 = [0.0, 1.0, 64.0]
SHIFTS5 = [0.0, 0.25, 1.0, 16.0, 1024.0]
COUNTS_F64 = [26, 26, 25, 22, 16, 10, 7, 4]


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


@pytest.fixture(autouse=True)
def _restore_poll(sa):
    ctx = sa.default_ctx(0)
    poll = ctx.get("poll")
    yield
    ctx.set("poll", poll)


def _is_single(dt):
    return np.dtype(dt) in (np.dtype(F32), np.dtype(C32))


def _tol(dt):
    return 1e-5 if _is_single(dt) else 1e-10


_sys_cache, _ref_cache = {}, {}


def _system(name, dt):
    """-> (ip, ix, d, rhs) in the dtype under test.  banded: test_gpu_cg_many.py's systems; p3d: 1287 rows, odd (a scalar tail, a
    padded last pack, several workgroups); tiny: 3 rows, fewer than one pack per lane."""
    key = (name, np.dtype(dt).name)
    if key not in _sys_cache:
        from sprsolve_amd import gen
        cx = np.dtype(dt).kind == "c"
        if name == "banded":
            ip, ix, d, rhs = gen.hermitian_banded(1500, 3) if cx else gen.symmetric_banded(2000)
        elif name == "p3d":
            ip, ix, d, rhs = gen.poisson3d(13, 11, 9)
        else:
            ip, ix = np.array([0, 2, 5, 7], np.int32), np.array([0, 1, 0, 1, 2, 1, 2], np.int32)
            d, rhs = np.array([4.0, -1, -1, 4, -1, -1, 4]), np.array([1.0, 2, 3])
        _sys_cache[key] = (ip, ix, d.astype(dt), rhs.astype(dt))
    return _sys_cache[key]


def _checker(name, dt, shifts):
    key = (name, np.dtype(dt).name, tuple(shifts))
    if key not in _ref_cache:
        ip, ix, d, rhs = _system(name, dt)
        _ref_cache[key] = shift.cg_shift(ip, ix, d, rhs, shifts, MAX_ITER, _tol(dt))
    return _ref_cache[key]


def _true_res(ip, ix, d, sigma, b, x):
    import scipy.sparse as sp
    wide = np.complex128 if d.dtype.kind == "c" else np.float64
    n = ip.size - 1
    M = sp.csr_matrix((d.astype(wide), ix, ip), shape=(n, n))
    xw = x.astype(wide)
    return np.linalg.norm(b.astype(wide) - (M @ xw + sigma * xw)) / np.linalg.norm(b.astype(wide))


def _assert_columns(name, dt, shifts, got):
    """Every column of one solve against the checker's, with the margins of tests/test_gpu_cg_many.py."""
    ip, ix, d, rhs = _system(name, dt)
    its, res, st, X = got
    cits, cres, cst, cX = _checker(name, dt, shifts)
    assert np.all(cst == ref.OK)
    tol = _tol(dt)
    for j, sg in enumerate(shifts):
        err = np.max(np.abs(X[j] - cX[j])); true = _true_res(ip, ix, d, sg, rhs, X[j])
        print("%s %s m=%d sigma %g: its %d (checker %d) res %.3e (checker %.3e) true %.3e max|x - checker| %.3e"
              % (name, np.dtype(dt).name, len(shifts), sg, its[j], cits[j], res[j], cres[j], true, err))
        assert st[j] == ref.OK
        assert abs(int(its[j]) - int(cits[j])) <= max(5, int(cits[j]) // 4)
        assert res[j] <= tol and true <= 10 * tol
        if _is_single(dt):
            assert err < (5e-3 if np.dtype(dt).kind == "c" else 2e-3)
        else:
            assert err <= 1e-7 * max(1.0, np.max(np.abs(cX[j])))


def _new(sa, name, dt, mmax):
    ip, ix, d, rhs = _system(name, dt)
    n = rhs.size
    A = sa.HipCsr.new((n, n), ip, ix, d)
    return A, sa.CGShift.new(A, n, mmax), rhs, n


def _run(s, shifts, rhs, n, dt, max_iter=MAX_ITER, tol=None):
    X = np.full((len(shifts), n), 7, dt)                         # x is output only: whatever it holds on entry is ignored
    its, res, st = s.solve(shifts, rhs, X, max_iter, _tol(dt) if tol is None else tol)
    return its, res, st, X


def _same(a, b):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. against the checker
@pytest.mark.parametrize("shifts", [SHIFTS, SHIFTS3], ids=["m8", "m3"])
@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_every_column_follows_the_checker(sa, dt, shifts):
    A, s, rhs, n = _new(sa, "banded", dt, len(shifts))
    got = _run(s, shifts, rhs, n, dt)                            # checker: at most 26 iterations
    _assert_columns("banded", dt, shifts, got)
    assert s.last_status == 0


# ------------------------------------------------------------------------------------------------ 2. bit identity inside the library
@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_a_column_sees_neither_its_neighbours_nor_poll(sa, dt):
    A, s, rhs, n = _new(sa, "banded", dt, 8)
    ctx = sa.default_ctx(0)
    alone = _run(s, [1.0], rhs, n, dt)
    last3 = _run(s, [0.0, 64.0, 1.0], rhs, n, dt)
    eight = _run(s, SHIFTS, rhs, n, dt)                          # sigma = 1 is the fourth of eight
    assert np.all(eight[2] == ref.OK) and np.all(last3[2] == ref.OK) and alone[2][0] == ref.OK
    for other, j in ((last3, 2), (eight, 3)):
        assert other[0][j] == alone[0][0] and other[1][j].tobytes() == alone[1][0].tobytes() and other[3][j].tobytes() == alone[3][0].tobytes()
    again = _run(s, SHIFTS, rhs, n, dt)                          # two consecutive solves on one handle
    assert _same(eight, again)
    ctx.set("poll", 1)
    p1 = _run(s, SHIFTS, rhs, n, dt)
    ctx.set("poll", 7)
    p7 = _run(s, SHIFTS, rhs, n, dt)
    assert _same(p1, p7) and _same(p1, eight)


# ------------------------------------------------------------------------------------------------ 3. frozen columns and events
def test_frozen_columns_and_events(sa):
    dt = F64
    ip, ix, d, rhs = _system("banded", dt)
    A, s, rhs, n = _new(sa, "banded", dt, 8)
    full = _run(s, SHIFTS, rhs, n, dt)
    assert np.all(full[2] == ref.OK) and s.last_status == 0
    # max_iter = 12: the columns whose count is below it return the bits of the unlimited run, the others stop there
    its, res, st, X = _run(s, SHIFTS, rhs, n, dt, max_iter=12)
    print("max_iter 12: its", its, "status", st, "unlimited", full[0])
    slow = [j for j in range(8) if full[0][j] > 12]
    fast = [j for j in range(8) if full[0][j] <= 12]
    assert slow == [j for j, c in enumerate(COUNTS_F64) if c > 12] and fast            # the same columns as the tabulated counts
    for j in fast:
        assert st[j] == ref.OK and its[j] == full[0][j] and res[j].tobytes() == full[1][j].tobytes() and X[j].tobytes() == full[3][j].tobytes()
    for j in slow:
        assert st[j] == ref.INSUFFICIENT_ITER and its[j] == 12
    assert s.last_status == ref.INSUFFICIENT_ITER
    # -A: not positive definite along the first direction
    An = sa.HipCsr.new((n, n), ip, ix, -d)
    sn = sa.CGShift.new(An, n, 8)
    its, res, st, X = _run(sn, SHIFTS, rhs, n, dt)
    assert np.all(st == ref.BREAKDOWN) and not np.any(its) and not np.any(X) and sn.last_status == ref.BREAKDOWN
    # a zero right-hand side, and a tolerance that the start already meets
    its, res, st, X = _run(s, SHIFTS, np.zeros(n, dt), n, dt)
    assert np.all(st == ref.OK) and not np.any(its) and not np.any(X) and s.last_status == 0
    its, res, st, X = _run(s, SHIFTS, rhs, n, dt, tol=2.0)
    assert np.all(st == ref.OK) and not np.any(its) and not np.any(X) and np.all(res == 1.0)


# ------------------------------------------------------------------------------------------------ 4. shapes
@pytest.mark.parametrize("dt", [F64, C32], ids=lambda d: np.dtype(d).name)
def test_odd_rows_and_five_shifts(sa, dt):
    """1287 rows: a scalar tail behind the packs (f64: 643 packs + 1 row; c32 likewise), a caller's block whose columns are not
    16-byte aligned (so x goes through the solver's own block), three workgroups.  Host arrays and a device vector."""
    A, s, rhs, n = _new(sa, "p3d", dt, 5)
    got = _run(s, SHIFTS5, rhs, n, dt)                           # checker: at most 45 iterations
    _assert_columns("p3d", dt, SHIFTS5, got)
    dB, dX = sa.DevVec.from_numpy(rhs), sa.DevVec.from_numpy(np.full(5 * n, 7, dt))
    its, res, st = s.solve(SHIFTS5, dB, dX, MAX_ITER, _tol(dt))
    assert _same(got, (its, res, st, dX.to_numpy().reshape(5, n)))


@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_three_rows(sa, dt):
    A, s, rhs, n = _new(sa, "tiny", dt, 8)
    got = _run(s, SHIFTS, rhs, n, dt)                            # checker: 3 iterations
    _assert_columns("tiny", dt, SHIFTS, got)


def test_x_beyond_m_columns_is_untouched(sa):
    """mmax = 8, m = 2, through the _dev entry with x_len = 2 n on a longer buffer (2000 rows: x is written in place)."""
    from sprsolve_amd import _lib
    from sprsolve_amd.device import dev_ptr
    dt = F64
    A, s, rhs, n = _new(sa, "banded", dt, 8)
    dB, dX = sa.DevVec.from_numpy(rhs), sa.DevVec.from_numpy(np.full(8 * n + 64, 7, dt))
    sh = np.array([0.25, 16.0])
    its = (C.c_size_t * 2)(); res = (C.c_double * 2)(); st = (C.c_int * 2)()
    rc = _lib.lib().sprs_cgshift_solve_dev_d(s.h, sh.ctypes.data_as(C.POINTER(C.c_double)), 2, dev_ptr(dB), n, dev_ptr(dX), 2 * n, MAX_ITER,
                                             _tol(dt), its, res, st)
    sa.default_ctx(0).sync()
    out = dX.to_numpy()
    assert rc == 0 and list(st) == [0, 0] and np.all(out[2 * n:] == 7)
    host = _run(s, list(sh), rhs, n, dt)
    assert out[:2 * n].tobytes() == host[3].tobytes() and list(its) == list(host[0])


# ------------------------------------------------------------------------------------------------ 5. arguments and entry points
def test_arguments(sa):
    from sprsolve_amd.error import IncompatibleMatrixFormat
    dt = F64
    A, s, rhs, n = _new(sa, "banded", dt, 3)
    X = np.full((3, n), 3, dt)
    for bad in ([], [0.0, 1.0, 2.0, 3.0], [0.0, -1.0], [np.nan], [1.0, np.inf]):
        with pytest.raises(ValueError):
            s.solve(bad, rhs, np.full((max(len(bad), 1), n), 3, dt), MAX_ITER, 1e-10)
    with pytest.raises(ValueError, match="negative or not finite"):
        s.solve([0.0, -1.0], rhs, X[:2].copy(), MAX_ITER, 1e-10)
    with pytest.raises(IncompatibleMatrixFormat, match="matrix size"):
        s.solve(SHIFTS3, rhs[:-1], X, MAX_ITER, 1e-10)
    with pytest.raises(IncompatibleMatrixFormat, match="output vec"):
        s.solve(SHIFTS3, rhs, np.full((3, n - 1), 3, dt), MAX_ITER, 1e-10)
    with pytest.raises(IncompatibleMatrixFormat, match="output vec"):
        s.solve(SHIFTS3, rhs, np.full((2, n), 3, dt), MAX_ITER, 1e-10)
    assert np.all(X == 3)                                        # argument errors write nothing
    for mmax in (0, 9):
        with pytest.raises(ValueError):
            sa.CGShift.new(A, n, mmax)


@pytest.mark.parametrize("dt", [F64, C64], ids=lambda d: np.dtype(d).name)
def test_device_and_host_entry_points_agree(sa, dt):
    A, s, rhs, n = _new(sa, "banded", dt, 8)
    host = _run(s, SHIFTS3, rhs, n, dt)                          # m = 3 on a handle made for 8
    dB, dX = sa.DevVec.from_numpy(rhs), sa.DevVec.from_numpy(np.full(3 * n, 7, dt))
    its, res, st = s.solve(SHIFTS3, dB, dX, MAX_ITER, _tol(dt))
    assert np.all(st == ref.OK) and _same(host, (its, res, st, dX.to_numpy().reshape(3, n)))


def test_distributed_operator_is_refused(sa):
    import torch
    from sprsolve_amd import _lib, dist as sdist
    from test_gpu_dist import _self_halo_plan
    ctx = sa.default_ctx(0)
    dev = torch.device("cuda", 0)
    comm = sdist.Comm(ctx, 0, 1)
    try:
        ip, ix, d, rhs = _system("banded", F64)
        n = ip.size - 1
        plan = _self_halo_plan(torch, dev, n, ix, lambda c: np.zeros(c.shape, bool))
        A = sdist.DistCsr.from_plan(comm, plan, int(ip[-1]), torch.from_numpy(ip.copy()).to(dev), torch.from_numpy(d.copy()).to(dev), adopt=True,
                                    to_device=lambda a: torch.from_numpy(a).to(dev))
        h = C.c_void_p()
        st = _lib.lib().sprs_cgshift_create_d(A.h, n, 4, C.byref(h))
        text = _lib.lib().sprs_last_error(ctx.h).decode()
        assert st == _lib.INVALID_ARGUMENT and not h.value and "distributed" in text, (st, text)
        with pytest.raises(ValueError, match="distributed"):
            sa.CGShift.new(A, n, 4)
    finally:
        comm.close()
