"""sprs_csr_adjoint / HipCsr.adjoint (csrc/transpose.hip): the handle built on the device against the handle the host conversion
builds from the same arrays passed as CSC with the dimensions swapped (sprs_csr_create_*, storage_csc = 1).  The two hold the same
arrays, so every SpMV through them agrees bit for bit whatever route the library picks; numpy's A.conj().T @ x is the
independent check of the values (to rounding: its sums associate differently)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
_ids = lambda v: np.dtype(v).name if isinstance(v, type) else str(v)


@pytest.fixture(scope="module")
def sa():
    import sprsolve_amd
    from sprsolve_amd import _lib
    _lib.lib()
    sprsolve_amd.default_ctx(0)
    return sprsolve_amd


@pytest.fixture(autouse=True)
def _restore_knobs(sa):
    yield
    sa.default_ctx(0).set("spmv_dict", -1)


def _values(rng, k, dt):
    v = rng.uniform(-1, 1, k)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.uniform(-1, 1, k)
    return v.astype(dt)


def _random_csr(m, n, dt, seed, per_row=4, empty_rows=(), empty_cols=(), dup=False):
    """Ragged rows of 0 .. 2 per_row entries in ascending column order; dup: every third row repeats one of its columns."""
    rng = np.random.default_rng(seed)
    cols_ok = np.setdiff1d(np.arange(n), np.asarray(empty_cols, dtype=int))
    rows = []
    for i in range(m):
        k = 0 if (i in empty_rows or cols_ok.size == 0) else int(rng.integers(0, 2 * per_row + 1))
        c = np.sort(rng.choice(cols_ok, size=min(k, cols_ok.size), replace=False))
        if dup and i % 3 == 0 and c.size:
            c = np.sort(np.concatenate([c, c[:1], c[-1:]]))
        rows.append(c)
    ip = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    ix = (np.concatenate(rows) if ip[-1] else np.zeros(0)).astype(np.int32)
    return ip, ix, _values(rng, int(ip[-1]), dt)


def _grid(nx, ny, dt, upwind):
    """5-point stencil with constant coefficients: the symmetric Laplacian, or a first-order upwind operator (west and south
    neighbours only), which is not symmetric."""
    import scipy.sparse as sp
    ex, ey = np.ones(nx), np.ones(ny)
    if upwind:
        Tx = sp.diags([-ex[:-1], 1.5 * ex], [-1, 0]); Ty = sp.diags([-0.5 * ey[:-1], 1.5 * ey], [-1, 0])
    else:
        Tx = sp.diags([-ex[:-1], 2 * ex, -ex[:-1]], [-1, 0, 1]); Ty = sp.diags([-ey[:-1], 2 * ey, -ey[:-1]], [-1, 0, 1])
    M = (sp.kron(sp.eye(ny), Tx) + sp.kron(Ty, sp.eye(nx))).tocsr()
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(dt)


def _host_adjoint(sa, shape, ip, ix, d, conjugate=True):
    """The checker: A's arrays as the CSC of the adjoint."""
    vals = d.conj() if (conjugate and d.dtype.kind == "c") else d
    return sa.HipCsr.new((shape[1], shape[0]), ip, ix, np.ascontiguousarray(vals), storage="CSC")


def _mul(sa, H, x):
    xd = sa.DevVec.from_numpy(x); yd = sa.DevVec(H.rows(), H.dtype)
    H.mul_vec_unchecked(xd, yd)
    return yd.to_numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check(sa, shape, ip, ix, d, conjugate=True, seed=0):
    m, n = shape
    A = sa.HipCsr.new(shape, ip, ix, d)
    G = A.adjoint(conjugate)
    W = _host_adjoint(sa, shape, ip, ix, d, conjugate)
    assert G.shape == W.shape == (n, m) and G.nnz() == W.nnz() == d.size
    for a, b in zip(G.to_host(), W.to_host()):
        assert np.array_equal(_bits(a), _bits(b))
    assert G.stream_format() == W.stream_format()
    assert G.spmv_route() == W.spmv_route()
    if m == 0 or n == 0:
        return A, G, None
    x = _values(np.random.default_rng(seed + 99), m, d.dtype)
    y, yw = _mul(sa, G, x), _mul(sa, W, x)
    assert np.array_equal(_bits(y), _bits(yw))
    import scipy.sparse as sp
    wide = C64 if d.dtype.kind == "c" else F64
    M = sp.csr_matrix((d.astype(wide), ix, ip), shape=shape)
    want = (M.conj().T if conjugate else M.T) @ x.astype(wide)
    # the worst-case rounding error of a sum of L products: (L + 4) eps sum |a_i x_i| per row, twice that for complex products
    L = int(np.max(np.bincount(ix, minlength=n))) if ix.size else 0
    bound = 2 * (L + 4) * np.finfo(d.dtype).eps * (abs(M).T @ np.abs(x.astype(wide)))
    assert np.all(np.abs(y - want) <= bound)
    return A, G, y


SHAPES = [(63, 67), (64, 67), (65, 67), (129, 67), (67, 63), (67, 64), (67, 65), (67, 129)]


@pytest.mark.parametrize("knob", [0, -1], ids=["csr", "auto"])
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_random_shapes(sa, dt, knob):
    sa.default_ctx(0).set("spmv_dict", knob)
    for k, shape in enumerate(SHAPES):
        ip, ix, d = _random_csr(shape[0], shape[1], dt, seed=k)
        _check(sa, shape, ip, ix, d, seed=k)


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_degenerate_and_ragged(sa, dt):
    z = np.zeros(0, np.int32)
    _check(sa, (0, 0), np.zeros(1, np.int32), z, np.zeros(0, dt))
    _check(sa, (5, 7), np.zeros(6, np.int32), z, np.zeros(0, dt))                       # nnz = 0
    _check(sa, (1, 1), np.array([0, 1], np.int32), np.zeros(1, np.int32), _values(np.random.default_rng(1), 1, dt))
    ip, ix, d = _random_csr(130, 67, dt, seed=3, empty_rows=(0, 5, 64, 129), empty_cols=(0, 1, 33, 66))
    _check(sa, (130, 67), ip, ix, d)
    ip, ix, d = _random_csr(65, 67, dt, seed=4, dup=True)                               # duplicates keep their stored order
    assert (np.diff(ix) == 0).any()
    _check(sa, (65, 67), ip, ix, d)


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_long_row_of_the_adjoint(sa, dt):
    """One column of 200 entries: the adjoint has a row over 96 entries, the wavefront-per-row block route, on both handles."""
    m, n = 300, 67
    ip, ix, d = _random_csr(m, n, dt, seed=8, empty_cols=(11,))
    rows = [np.sort(np.append(ix[ip[i]:ip[i + 1]], 11)) if i < 200 else ix[ip[i]:ip[i + 1]] for i in range(m)]
    ip2 = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int32)
    ix2 = np.concatenate(rows).astype(np.int32)
    d2 = _values(np.random.default_rng(9), ix2.size, dt)
    _, G, _ = _check(sa, (m, n), ip2, ix2, d2)
    gp = G.to_host()[0]
    assert gp[12] - gp[11] == 200


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_stencils(sa, dt):
    nx = ny = 32
    ip, ix, d = _grid(nx, ny, dt, upwind=False)
    A, G, y = _check(sa, (nx * ny, nx * ny), ip, ix, d)
    x = _values(np.random.default_rng(99), nx * ny, dt)            # the x of _check (seed 0 + 99)
    assert np.array_equal(_bits(y), _bits(_mul(sa, A, x)))        # A^T = A: the same operator, the same bits
    assert G.stream_format() == A.stream_format()
    if np.dtype(dt) == np.dtype(F64):
        assert G.stream_format()[0] == 2                          # (offset, value) pair codes
    ip, ix, d = _grid(nx, ny, dt, upwind=True)
    A, G, y = _check(sa, (nx * ny, nx * ny), ip, ix, d)
    assert not np.array_equal(_bits(y), _bits(_mul(sa, A, x)))
    if np.dtype(dt) == np.dtype(F64):
        assert G.stream_format()[0] == 2


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_adjoint_of_the_adjoint_and_determinism(sa, dt):
    shape = (129, 67)
    ip, ix, d = _random_csr(*shape, dt, seed=12, dup=True)
    A = sa.HipCsr.new(shape, ip, ix, d)
    G1, G2 = A.adjoint(), A.adjoint()
    for a, b in zip(G1.to_host(), G2.to_host()):
        assert np.array_equal(_bits(a), _bits(b))
    B = G1.adjoint()
    assert B.shape == A.shape
    for a, b in zip(B.to_host(), A.to_host()):                    # rows in ascending column order with stable duplicates: A itself
        assert np.array_equal(_bits(a), _bits(b))
    x = _values(np.random.default_rng(13), shape[1], dt)
    assert np.array_equal(_bits(_mul(sa, B, x)), _bits(_mul(sa, A, x)))


@pytest.mark.parametrize("dt", [C64, C32], ids=_ids)
def test_conjugate_on_and_off(sa, dt):
    shape = (65, 67)
    ip, ix, d = _random_csr(*shape, dt, seed=14)
    _, GH, yh = _check(sa, shape, ip, ix, d, conjugate=True)
    _, GT, yt = _check(sa, shape, ip, ix, d, conjugate=False)
    vh, vt = GH.to_host()[2], GT.to_host()[2]
    assert np.array_equal(_bits(vh.real), _bits(vt.real)) and np.array_equal(_bits(vh.imag), _bits(-vt.imag))
    assert not np.array_equal(_bits(yh), _bits(yt))


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_mul_mat_through_the_adjoint(sa, dt):
    shape = (129, 67)
    ip, ix, d = _random_csr(*shape, dt, seed=15)
    G = sa.HipCsr.new(shape, ip, ix, d).adjoint()
    X = _values(np.random.default_rng(16), shape[0] * 3, dt).reshape(shape[0], 3)
    Y = np.empty((shape[1], 3), dt)
    G.mul_mat(X, Y)
    for c in range(3):
        assert np.array_equal(_bits(Y[:, c]), _bits(_mul(sa, G, np.ascontiguousarray(X[:, c]))))


def test_real_dtypes_ignore_the_flag(sa):
    ip, ix, d = _random_csr(65, 67, F64, seed=17)
    A = sa.HipCsr.new((65, 67), ip, ix, d)
    for a, b in zip(A.adjoint(True).to_host(), A.adjoint(False).to_host()):
        assert np.array_equal(_bits(a), _bits(b))
