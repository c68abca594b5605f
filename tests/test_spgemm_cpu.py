"""The CSR x CSR product (sprs_csr_matmul) without a GPU: the symbol is exported and mirrored, HipCsr has the two methods, and the
checker the GPU file compares against (tests/_amg_ref.py::spgemm) agrees with a dense product on integer-valued matrices, where
every sum is exact whatever its order — including an entry whose terms cancel to zero and must stay stored."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _amg_ref as amg  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from sprsolve_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_library_exports_matmul_and_the_binding_lists_it(L):
    from sprsolve_amd import _lib
    assert hasattr(L, "sprs_csr_matmul")
    assert "sprs_csr_matmul" in _lib.all_symbols()
    assert len(_lib.PROTOTYPES["sprs_csr_matmul"]) == 4
    assert L.sprs_csr_matmul(None, None, None, None) == _lib.INVALID_ARGUMENT      # null handles never reach the device


def test_hipcsr_has_matmul_and_the_operator():
    from sprsolve_amd import HipCsr
    assert callable(getattr(HipCsr, "matmul", None))
    assert callable(getattr(HipCsr, "__matmul__", None))
    A = HipCsr(None, None, np.float64, (2, 3))                                     # no handle: only the dispatch is looked at
    assert A.__matmul__(np.zeros((3, 2))) is NotImplemented
    with pytest.raises(TypeError):
        A.matmul(np.zeros((3, 2)))


def _csr(M, keep=None):
    """CSR arrays of a dense matrix: the non-zeros, plus the positions of `keep` stored as they are."""
    mask = M != 0
    if keep is not None:
        mask = mask | keep
    ip = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    r, c = np.nonzero(mask)
    return ip, c.astype(np.int32), M[r, c]


@pytest.mark.parametrize("dt", [np.float64, np.complex128, np.float32, np.complex64], ids=lambda d: np.dtype(d).name)
def test_checker_equals_the_dense_product_on_integer_matrices(dt):
    rng = np.random.default_rng(5)
    A = rng.integers(-3, 4, (7, 5)) * (rng.random((7, 5)) < 0.5)
    B = rng.integers(-3, 4, (5, 6)) * (rng.random((5, 6)) < 0.5)
    A = A.astype(dt); B = B.astype(dt)
    if np.dtype(dt).kind == "c":
        A = A + 1j * np.roll(A.real, 1, axis=0); B = B - 1j * np.roll(B.real, 1, axis=1)
        A = A.astype(dt); B = B.astype(dt)
    op = amg.Ops(dt)
    cp, cx, cv = amg.spgemm(op, 6, *_csr(A), *_csr(B))
    D = A @ B
    structural = ((A != 0).astype(int) @ (B != 0).astype(int)) > 0
    rows = np.repeat(np.arange(7), np.diff(cp))
    got = np.zeros((7, 6), dt); got[rows, cx] = cv
    seen = np.zeros((7, 6), bool); seen[rows, cx] = True
    assert np.array_equal(seen, structural)                  # the structural pattern, nothing dropped
    assert np.array_equal(got, D)
    for i in range(7):
        assert np.all(np.diff(cx[cp[i]:cp[i + 1]]) > 0)


def test_checker_keeps_an_entry_that_cancels_exactly():
    # row 0 of A meets column 1 of B through k = 0 and k = 2: 2 * 3 + (-3) * 2 = 0, and the entry stays
    A = np.array([[2.0, 0.0, -3.0], [0.0, 1.0, 0.0]])
    B = np.array([[0.0, 3.0], [4.0, 0.0], [5.0, 2.0]])
    op = amg.Ops(np.float64)
    cp, cx, cv = amg.spgemm(op, 2, *_csr(A), *_csr(B))
    assert cp.tolist() == [0, 2, 3] and cx.tolist() == [0, 1, 0]
    assert cv.tolist() == [-15.0, 0.0, 4.0]
    assert not np.signbit(cv[1])
    assert np.array_equal((A @ B)[[0, 0, 1], [0, 1, 0]], cv)
