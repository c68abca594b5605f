"""CSR SpMM (sprs_mul_mat_*, csrc/spmm.hip): column c of Y = A X must carry the BITS of mul_vec on column c of X — every
dtype, every K instantiation (k = 1, 2 exact; 3 -> K 4 and 5 -> K 8 through the masked element-wise gather; 8 exact), stream
and vector row blocks, special values, the host and the device entry points and their argument checks."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
KS = [1, 2, 3, 5, 8]


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


def _values(seed, n, dt):
    from sprsolve_amd import gen
    v = gen.uniform(gen.SEED + seed, n)
    if np.dtype(dt).kind == "c":
        v = v + 1j * gen.uniform(gen.SEED + seed, n, stream=1)
    return v.astype(dt)


def _ragged(dt):
    """1000 x 1300 (1000 is no multiple of 64): empty rows, one-entry rows, rows of 2 .. 12 entries, and row 500 with 700
    entries — a row longer than a 508-entry stream block, i.e. a wavefront-per-row block between lane-per-row ones."""
    rng = np.random.RandomState(12345)
    nr, nc = 1000, 1300
    lens = rng.randint(2, 13, size=nr)
    lens[::7] = 0; lens[3::11] = 1; lens[500] = 700; lens[nr - 1] = 5
    ip = np.zeros(nr + 1, np.int32); ip[1:] = np.cumsum(lens)
    ix = np.concatenate([np.sort(rng.choice(nc, size=l, replace=False)) for l in lens]).astype(np.int32)
    return (nr, nc), ip, ix, _values(11, ix.size, dt)


def _banded(dt):
    from sprsolve_amd import gen
    ip, ix, d, _ = gen.symmetric_banded(2000)
    return (2000, 2000), ip, ix, (d.astype(dt) * (1 + 0.25j) if np.dtype(dt).kind == "c" else d.astype(dt))


def _tiny(dt):
    ip = np.array([0, 2, 2, 5], np.int32); ix = np.array([0, 2, 0, 1, 2], np.int32)
    return (3, 3), ip, ix, _values(13, 5, dt)


CASES = {"ragged": _ragged, "banded": _banded, "tiny": _tiny}
_cache = {}


def _columns(sa, case, dt):
    """-> (A, X (ncols, 8), Y1 (nrows, 8)): the matrix, eight input columns and mul_vec of each — computed once per (case, dtype)."""
    key = (case, np.dtype(dt).name)
    if key not in _cache:
        shape, ip, ix, d = CASES[case](dt)
        A = sa.HipCsr.new(shape, ip, ix, d)
        X = np.stack([_values(20 + c, shape[1], dt) for c in range(8)], axis=1)
        Y1 = np.zeros((shape[0], 8), dt)
        for c in range(8):
            y = np.zeros(shape[0], dt)
            A.mul_vec(np.ascontiguousarray(X[:, c]), y) if shape[0] == shape[1] else _mul_vec_rect(sa, A, np.ascontiguousarray(X[:, c]), y)
            Y1[:, c] = y
        _cache[key] = (A, X, Y1)
    return _cache[key]


def _mul_vec_rect(sa, A, x, y):
    """mul_vec's host entry wants a square matrix (mat.rs:50-52); a rectangular one goes through the device entry."""
    dx, dy = sa.DevVec.from_numpy(x), sa.DevVec(y.size, y.dtype)
    A.mul_vec_unchecked(dx, dy)
    y[:] = dy.to_numpy()


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", sorted(CASES))
def test_columns_carry_mul_vec_bits(sa, case, dt, k):
    A, X, Y1 = _columns(sa, case, dt)
    Xk = np.ascontiguousarray(X[:, :k])
    Y = np.full((A.rows(), k), 7, dt)
    A.mul_mat(Xk, Y)
    assert np.any(Y1[:, :k] != 0)
    assert _same_bits(Y, np.ascontiguousarray(Y1[:, :k]))
    # the device entry on the same block: the same bits
    dX, dY = sa.DevVec.from_numpy(Xk.ravel()), sa.DevVec(A.rows() * k, dt)
    A.mul_mat(dX, dY)
    assert _same_bits(dY.to_numpy().reshape(A.rows(), k), Y)


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("dt", ALL, ids=lambda d: np.dtype(d).name)
def test_special_values_stay_in_their_column(sa, dt, k):
    """+-0.0 anywhere and a NaN in ONE column: that column follows mul_vec's bits (NaN pattern included), every other column
    is bit-identical to what it is without the NaN."""
    A, X, _ = _columns(sa, "ragged", dt)
    Xk = np.ascontiguousarray(X[:, :k])
    Xk[::5, :] = 0.0; Xk[1::5, :] = -0.0
    clean = np.zeros((A.rows(), k), dt)
    A.mul_mat(Xk, clean)
    bad = Xk.copy(); bad[A.cols() // 2, k - 2] = np.nan; bad[7, k - 2] = np.nan
    Y = np.zeros((A.rows(), k), dt)
    A.mul_mat(bad, Y)
    others = [c for c in range(k) if c != k - 2]
    assert _same_bits(np.ascontiguousarray(Y[:, others]), np.ascontiguousarray(clean[:, others]))
    assert np.isnan(Y[:, k - 2]).any() and not np.isnan(Y[:, others]).any()
    for c in range(k):
        y = np.zeros(A.rows(), dt)
        _mul_vec_rect(sa, A, np.ascontiguousarray(bad[:, c]), y)
        assert _same_bits(np.ascontiguousarray(Y[:, c]), y)


def test_argument_checks(sa):
    from sprsolve_amd import _lib
    L = _lib.lib()
    A, X, _ = _columns(sa, "ragged", F64)
    nr, nc = A.rows(), A.cols()
    x = np.zeros(nc * 9); y = np.full(nr * 9, 5.0)
    xp, yp = x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)
    assert L.sprs_mul_mat_d(A.h, xp, nc * 3, yp, nr * 3, 3) == _lib.OK
    assert L.sprs_mul_mat_d(A.h, xp, nc * 3 + 1, yp, nr * 3, 3) == _lib.DIM_MISMATCH          # wrong x_len
    assert L.sprs_mul_mat_d(A.h, xp, nc * 3, yp, nr * 2, 3) == _lib.DIM_MISMATCH              # wrong y_len
    assert L.sprs_mul_mat_d(A.h, xp, nr * 3, yp, nr * 3, 3) == _lib.DIM_MISMATCH              # x sized by the rows of a 1000 x 1300 matrix
    for k in (0, 9):
        assert L.sprs_mul_mat_d(A.h, xp, nc * k, yp, nr * k, k) == _lib.INVALID_ARGUMENT
        dX, dY = sa.DevVec(nc * 9, F64), sa.DevVec(nr * 9, F64)
        assert L.sprs_mul_mat_dev_d(A.h, dX.ptr, dY.ptr, k) == _lib.INVALID_ARGUMENT
    assert L.sprs_mul_mat_z(A.h, xp, nc * 2, yp, nr * 2, 2) == _lib.INVALID_ARGUMENT         # a handle of another scalar type
    assert L.sprs_mul_mat_dev_s(A.h, xp, yp, 2) == _lib.INVALID_ARGUMENT
    assert L.sprs_mul_mat_d(None, xp, nc, yp, nr, 1) == _lib.INVALID_ARGUMENT
    from sprsolve_amd.error import DimensionMismatch
    with pytest.raises(DimensionMismatch):
        A.mul_mat(np.zeros((nc, 2)), np.zeros((nr, 3)))
    with pytest.raises(TypeError):
        A.mul_mat(np.zeros(nc), np.zeros(nr))
