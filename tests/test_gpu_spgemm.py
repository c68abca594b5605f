"""The CSR x CSR product on the GPU (sprs_csr_matmul, csrc/spgemm.hip) against tests/_amg_ref.py::spgemm, the numpy statement of
the serial row-by-row loop.  Every comparison is exact: indptr and indices equal, values as raw bits; where an operand holds NaN,
NaN at the same positions and bits elsewhere.  `info` (rows per kernel and the two limits) is what the cases use to reach every
kernel and both sides of both limits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _amg_ref as amg  # noqa: E402
from test_amg_cpu import system_of  # noqa: E402

pytestmark = pytest.mark.gpu

F64, C64, F32, C32 = np.float64, np.complex128, np.float32, np.complex64
ALL = [F64, C64, F32, C32]
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


def parts(a):
    a = np.ascontiguousarray(a)
    return a.view(a.real.dtype) if a.dtype.kind == "c" else a


def reference(ncols, A, B):
    with np.errstate(all="ignore"):
        cp, cx, cv = amg.spgemm(amg.Ops(A[2].dtype), ncols, *[np.asarray(v) for v in A], *[np.asarray(v) for v in B])
    return cp, cx, cv


def same(got, want, nan=False):
    gp, gx, gv = got
    wp, wx, wv = want
    assert np.array_equal(gp, wp) and np.array_equal(gx, wx)
    assert gv.dtype == wv.dtype
    if not nan:
        assert np.array_equal(bits(gv), bits(wv))
        return
    g, w = parts(gv), parts(wv)
    assert np.array_equal(np.isnan(g), np.isnan(w))
    ok = ~np.isnan(w)
    assert np.array_equal(bits(g[ok]), bits(w[ok]))


def product(sa, shape_a, A, shape_b, B, nan=False):
    """C = A B on the device, compared with the checker -> (C, info, the checker's arrays)."""
    Ah = sa.HipCsr.new(shape_a, *A)
    Bh = sa.HipCsr.new(shape_b, *B)
    Ch, info = Ah.matmul(Bh, info=True)
    assert Ch.shape == (shape_a[0], shape_b[1]) and Ch.dtype == np.dtype(A[2].dtype)
    assert sum(info[:3]) == shape_a[0]
    want = reference(shape_b[1], A, B)
    assert Ch.nnz() == int(want[0][-1])
    same(Ch.to_host(), want, nan)
    return Ch, info, want


def values(rng, n, dt):
    """Values with a full mantissa, so that the order of a sum shows in its last bit."""
    v = rng.uniform(-1.0, 1.0, n)
    if np.dtype(dt).kind == "c":
        v = v + 1j * rng.uniform(-1.0, 1.0, n)
    return v.astype(dt)


def ragged(rng, nrows, ncols, lengths, dt):
    """CSR arrays with the given row lengths, columns strictly ascending."""
    ip = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    ix = np.concatenate([np.sort(rng.choice(ncols, int(m), replace=False)) for m in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ip, ix, values(rng, ix.size, dt)


# ------------------------------------------------------------------------------------------------ 1. a stencil squared
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_stencil_squared_on_the_short_path(sa, dt):
    ip, ix, d, _ = system_of("p3_8x7x6", np.dtype(dt).name)
    n = ip.size - 1
    Ch, info, _ = product(sa, (n, n), (ip, ix, d), (n, n), (ip, ix, d))
    assert info[0] == n and info[1] == 0 and info[2] == 0          # 7 entries times 7: u_i <= 49


# ------------------------------------------------------------------------------------------------ 2. rectangular and ragged
@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_rectangular_ragged_with_empty_rows(sa, dt):
    rng = np.random.default_rng(11)
    lb = rng.integers(0, 5, 200); lb[:20] = 0                                     # rows 0..19 of B are empty
    B = ragged(rng, 200, 150, lb, dt)
    la = rng.integers(0, 6, 300); la[[0, 17, 299]] = 0                            # empty rows of A
    ip = np.concatenate([[0], np.cumsum(la)]).astype(np.int32)
    cols = [np.sort(rng.choice(200, int(m), replace=False)) for m in la]
    cols[5] = np.sort(rng.choice(20, la[5] if la[5] else 2, replace=False))       # row 5 meets empty rows of B only
    la[5] = cols[5].size
    ip = np.concatenate([[0], np.cumsum(la)]).astype(np.int32)
    ix = np.concatenate(cols).astype(np.int32)
    A = (ip, ix, values(rng, ix.size, dt))
    Ch, info, want = product(sa, (300, 200), A, (200, 150), B)
    lens = np.diff(want[0])
    assert lens[0] == 0 and lens[5] == 0 and lens[299] == 0 and lens.max() > 4
    assert info[0] == 300


# ------------------------------------------------------------------------------------------------ 3. A in any stored order
@pytest.mark.parametrize("dt", [F64, C32], ids=_ids)
def test_left_operand_unsorted_with_duplicate_columns(sa, dt):
    rng = np.random.default_rng(12)
    B = ragged(rng, 50, 40, rng.integers(1, 9, 50), dt)
    la = rng.integers(2, 9, 60)
    ip = np.concatenate([[0], np.cumsum(la)]).astype(np.int32)
    ix = rng.integers(0, 50, ip[-1]).astype(np.int32)                             # any order, repeats included
    ix[ip[3]:ip[3] + 2] = 7                                                       # a sure duplicate
    assert any(np.any(np.diff(ix[ip[i]:ip[i + 1]]) < 0) for i in range(60))
    A = (ip, ix, values(rng, ix.size, dt))
    Ch, info, want = product(sa, (60, 50), A, (50, 40), B)
    # the fold follows A's stored order: the same row sorted by column gives other bits somewhere
    order = np.lexsort((ix, np.repeat(np.arange(60), la)))
    other = reference(40, (ip, ix[order], A[2][order]), B)
    assert np.array_equal(other[1], want[1]) and not np.array_equal(bits(other[2]), bits(want[2]))


# ------------------------------------------------------------------------------------------------ 4. the table path
def table_case(dt):
    rng = np.random.default_rng(13)
    lb = np.full(80, 20)
    bp = np.concatenate([[0], np.cumsum(lb)]).astype(np.int32)
    bx = np.concatenate([np.sort(rng.choice(60, 20, replace=False)) for _ in range(80)]).astype(np.int32)     # 20 of 60 columns: heavy overlap
    bv = values(rng, bx.size, dt)
    bx[20:40] = bx[0:20]; bv[20:40] = bv[0:20]                                    # rows 0 and 1 of B are equal
    ap = (30 * np.arange(41)).astype(np.int32)
    ax = np.concatenate([np.sort(rng.choice(80, 30, replace=False)) for _ in range(40)]).astype(np.int32)
    av = values(rng, ax.size, dt)
    ax[:30] = np.tile([0, 1], 15)                                                 # row 0 of A: fifteen pairs (v, -v) on equal rows
    av[:30:2] = av[1:30:2]; av[1:30:2] = -av[:30:2]
    return (ap, ax, av), (bp, bx, bv)


@pytest.mark.parametrize("dt", ALL, ids=_ids)
def test_table_path_with_overlap_and_exact_cancellation(sa, dt):
    A, B = table_case(dt)
    Ch, info, want = product(sa, (40, 80), A, (80, 60), B)
    assert info[1] == 40 and info[0] == 0 and info[2] == 0                        # u_i = 600
    cp, cx, cv = want
    assert cp[1] == 20 and np.all(parts(cv[:20]) == 0) and not np.any(np.signbit(parts(cv[:20])))    # cancelled, stored, +0
    gp, gx, gv = Ch.to_host()
    assert gp[1] == 20 and not np.any(bits(gv[:20]))


# ------------------------------------------------------------------------------------------------ 5. both sides of both limits
@pytest.mark.parametrize("dt", [F64, F32, C64], ids=_ids)
def test_rows_at_and_just_above_each_limit(sa, dt):
    rng = np.random.default_rng(14)
    lb = np.full(65, 32); lb[64] = 1
    B = ragged(rng, 65, 4096, lb, dt)
    one = (np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1, dt))
    _, info0 = sa.HipCsr.new((1, 65), *one).matmul(sa.HipCsr.new((65, 4096), *B), info=True)
    short_max, table_max = info0[3], info0[4]
    assert info0[:3] == [1, 0, 0] and 32 <= short_max < table_max <= 64 * 32

    def row_of(u):                                                                # columns of a row of A whose bound is exactly u
        return [k for k in range(u // 32)] + [64] * (u % 32)
    want_path = {short_max: 0, short_max + 1: 1, table_max: 1, table_max + 1: 2}
    for u, path in want_path.items():
        cols = row_of(u)
        A = (np.array([0, len(cols)], np.int32), np.array(cols, np.int32), values(rng, len(cols), dt))
        Ch, info, _ = product(sa, (1, 65), A, (65, 4096), B)
        assert info[:3] == [int(path == p) for p in range(3)], (u, info)
    rows = [row_of(u) for u in want_path]                                         # and the four rows in one call
    ap = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    ax = np.concatenate(rows).astype(np.int32)
    Ch, info, _ = product(sa, (4, 65), (ap, ax, values(rng, ax.size, dt)), (65, 4096), B)
    assert info[:3] == [1, 2, 1] and info[3:] == [short_max, table_max]


# ------------------------------------------------------------------------------------------------ 6. the dense fallback
@pytest.mark.parametrize("dt", [F32, C64], ids=_ids)
def test_fallback_row_wider_than_any_lds_table(sa, dt):
    rng = np.random.default_rng(15)
    bp = (400 * np.arange(65)).astype(np.int32)
    bx = np.concatenate([320 * k + np.arange(400) for k in range(64)]).astype(np.int32)
    B = (bp, bx, values(rng, bx.size, dt))
    ap = np.array([0, 2, 66, 68], np.int32)
    ax = np.concatenate([[3, 10], rng.permutation(64), [5, 40]]).astype(np.int32)
    A = (ap, ax, values(rng, ax.size, dt))
    Ch, info, want = product(sa, (3, 64), A, (64, 32768), B)
    assert np.diff(want[0])[1] == 63 * 320 + 400 > 20480                          # more columns than 160 KiB hold at 8 bytes a slot
    assert info[2] >= 1 and info[1] == 2 and info[0] == 0


# ------------------------------------------------------------------------------------------------ 7. special values
@pytest.mark.parametrize("dt", [F64, C64], ids=_ids)
def test_special_values_and_the_sign_of_zero(sa, dt):
    rng = np.random.default_rng(16)
    B = ragged(rng, 30, 25, rng.integers(1, 6, 30), dt)
    A = ragged(rng, 20, 30, rng.integers(1, 6, 20), dt)
    bv = B[2].copy(); av = A[2].copy()
    bv[[1, 8, 20]] = [np.inf, -np.inf, np.nan]; bv[[3, 30]] = -0.0
    av[[2, 9]] = [np.inf, np.nan]; av[[5, 14]] = -0.0
    # row 19 of A: one entry, -1, onto row 29 of B: one entry, +0 -> the only product is -0.0, and +0.0 is stored
    ap, ax = A[0].copy(), A[1].copy()
    bp, bx = B[0].copy(), B[1].copy()
    keep_a, keep_b = ap[19], bp[29]
    ap[20] = keep_a + 1; ax = ax[:keep_a + 1].copy(); ax[keep_a] = 29; av = av[:keep_a + 1].copy(); av[keep_a] = -1.0
    bp[30] = keep_b + 1; bx = bx[:keep_b + 1].copy(); bx[keep_b] = 4; bv = bv[:keep_b + 1].copy(); bv[keep_b] = 0.0
    Ch, info, want = product(sa, (20, 30), (ap, ax, av), (30, 25), (bp, bx, bv), nan=True)
    assert np.isnan(parts(want[2])).any() and np.isinf(parts(want[2])).any()
    gp, gx, gv = Ch.to_host()
    assert gp[20] - gp[19] == 1 and gx[gp[19]] == 4
    assert not np.any(bits(gv[gp[19]:gp[20]]))                                   # +0.0 in every component


# ------------------------------------------------------------------------------------------------ 8. - 10. the result is an operator
def test_same_bytes_twice_and_the_result_multiplies_like_any_handle(sa):
    A, B = table_case(F64)
    Ah, Bh = sa.HipCsr.new((40, 80), *A), sa.HipCsr.new((80, 60), *B)
    C1, C2 = Ah.matmul(Bh), Ah @ Bh
    h1, h2 = C1.to_host(), C2.to_host()
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(h1, h2))
    ip, ix, d, _ = system_of("p3_8x7x6", "float64")                               # (the host mul_vec takes square operators)
    n = ip.size - 1
    Sh = sa.HipCsr.new((n, n), ip, ix, d)
    S2 = Sh @ Sh
    x = np.random.default_rng(17).uniform(-1, 1, n)
    y1, y2 = np.empty(n), np.empty(n)
    S2.mul_vec(x, y1)
    sa.HipCsr.new((n, n), *S2.to_host()).mul_vec(x, y2)
    assert np.array_equal(bits(y1), bits(y2)) and np.any(y1)


@pytest.mark.parametrize("dt", [F64, C32], ids=_ids)
def test_square_result_takes_adjoint_and_matmul(sa, dt):
    ip, ix, d, _ = system_of("p3_8x7x6", np.dtype(dt).name)
    n = ip.size - 1
    Ah = sa.HipCsr.new((n, n), ip, ix, d)
    Ch = Ah @ Ah                                                                  # A == B
    cp, cx, cv = Ch.to_host()
    tp, tx, tv = amg.transpose_conj(amg.Ops(dt), n, cp.astype(np.int64), cx.astype(np.int64), cv)
    same(Ch.adjoint().to_host(), (tp, tx, tv))
    C2, info = Ch.matmul(Ch, info=True)                                           # 25 entries times up to 25: the table kernel too
    same(C2.to_host(), reference(n, (cp, cx, cv), (cp, cx, cv)))
    assert info[1] > 0


# ------------------------------------------------------------------------------------------------ 11. errors
def test_errors(sa):
    from sprsolve_amd import _lib
    from sprsolve_amd.error import DimensionMismatch
    L = _lib.lib()
    rng = np.random.default_rng(18)
    A = sa.HipCsr.new((6, 5), *ragged(rng, 6, 5, np.full(6, 2), F64))
    B = sa.HipCsr.new((5, 7), *ragged(rng, 5, 7, np.full(5, 3), F64))
    with pytest.raises(DimensionMismatch):
        B.matmul(B)                                                               # 5 x 7 times 5 x 7
    h = C.c_void_p()
    assert L.sprs_csr_matmul(B.h, B.h, C.byref(h), None) == _lib.DIM_MISMATCH and not h.value
    B32 = sa.HipCsr.new((5, 7), *ragged(rng, 5, 7, np.full(5, 3), F32))
    with pytest.raises(ValueError, match="scalar type"):
        A.matmul(B32)
    assert L.sprs_csr_matmul(A.h, B32.h, C.byref(h), None) == _lib.INVALID_ARGUMENT and not h.value
    # one descending pair in row 3 of B, then a second one in row 1: the smallest row is named
    bp, bx, bv = [v.copy() for v in ragged(rng, 5, 7, np.full(5, 3), F64)]
    bx[bp[3]:bp[3] + 2] = bx[bp[3]:bp[3] + 2][::-1]
    with pytest.raises(ValueError, match=r"row 3 of the right operand"):
        A.matmul(sa.HipCsr.new((5, 7), bp, bx, bv))
    bx[bp[1] + 1] = bx[bp[1]]                                                     # equal neighbours are not strictly ascending either
    with pytest.raises(ValueError, match=r"row 1 of the right operand"):
        A.matmul(sa.HipCsr.new((5, 7), bp, bx, bv))
    for args in ((None, B.h, C.byref(h), None), (A.h, None, C.byref(h), None), (A.h, B.h, None, None)):
        assert L.sprs_csr_matmul(*args) == _lib.INVALID_ARGUMENT
    Ch = A.matmul(B)                                                              # and info = NULL is fine
    assert Ch.shape == (6, 7)


# ------------------------------------------------------------------------------------------------ 12. Galerkin through the public interface
@pytest.mark.parametrize("name,dt", [("p3_12x11x10", F64), ("cd24x20", C32)], ids=_ids)
def test_galerkin_product_equals_the_hierarchy(sa, name, dt):
    ip, ix, d, _ = system_of(name, np.dtype(dt).name)
    n = ip.size - 1
    Ah = sa.HipCsr.new((n, n), ip, ix, d)
    M = sa.AMG.new(Ah)
    nc = M.info["rows"][1]
    P = sa.HipCsr.new((n, nc), *M.level(0, "P"))
    R = sa.HipCsr.new((nc, n), *M.level(0, "R"))
    Ac = R @ (Ah @ P)
    assert Ac.shape == (nc, nc)
    got, want = Ac.to_host(), M.level(1, "A")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(bits(got[2]), bits(want[2]))
    M2 = sa.AMG.new(Ac, coarse_max=8)                                             # the product is an operator AMG.new takes
    assert M2.info["rows"][0] == nc
