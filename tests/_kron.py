"""Large test operators whose truth comes from small factors, never from the code under test and never from a dense matrix of the
big operator.

kron_sum:     A = I (x) T1 + T2 (x) I with Hermitian tridiagonal T1 (n1 x n1), T2 (n2 x n2): its spectrum is exactly
              {lambda_i(T1) + mu_j(T2)} and exp(t A) vec(V) = vec(E2 V E1^T) with E = expm(t T), V the (n2, n1) reshape of v.
              Each factor carries a few isolated eigenvalues at both ends above a dense cluster, so the extreme pairs of A are
              well separated whatever n2 is.
kron_product: B = B2 (x) B1 with small sparse rectangular factors: its singular values are the products sigma_i(B1) sigma_j(B2).
True residuals are formed in double with scipy.sparse."""
import functools

import numpy as np

F64, C64 = np.float64, np.complex128


def factor_bands(nf, tops, bots, lo, hi, off, cplx, seed):
    """-> (d, e), the diagonal and the upper off-diagonal of the Hermitian tridiagonal factor: d = linspace(lo, hi, nf) shuffled by
    default_rng(seed) with the entries at linspace(0, nf - 1, len(tops) + len(bots) + 2).astype(int)[1:-1] overwritten by
    tops + bots, e_k = off (real) or off exp(1j k) (complex)."""
    d = np.linspace(lo, hi, nf)
    np.random.default_rng(seed).shuffle(d)
    iso = list(tops) + list(bots)
    d[np.linspace(0, nf - 1, len(iso) + 2).astype(int)[1:-1]] = iso
    k = np.arange(nf - 1)
    return d, (off * np.exp(1j * k) if cplx else np.full(nf - 1, float(off)))


def factor(nf, tops, bots, lo, hi, off, cplx, seed):
    """-> T = tridiag(conj(e), d, e) of factor_bands, dense."""
    d, e = factor_bands(nf, tops, bots, lo, hi, off, cplx, seed)
    return np.diag(d.astype(C64 if cplx else F64)) + np.diag(e, 1) + np.diag(np.conj(e), -1)


_T1 = ([1, .5], [-1, -.5], 0, .1, .02)
_T2 = ([3, 2.2, 1.6], [-3, -2.2, -1.6], 0, .3, .03)


def factors(n1, n2, cplx):
    """The two factors, dense (for the exponentials of small ones)."""
    return factor(n1, *_T1, cplx, 1), factor(n2, *_T2, cplx, 2)


def _tridiag_eigvalsh(d, e):
    """The eigenvalues of tridiag(conj(e), d, e) from LAPACK's symmetric tridiagonal solver: with D = diag(1, u_0, u_0 u_1, ...),
    u_k = conj(e_k) / |e_k|, D^H T D is the real tridiag(|e|, d, |e|), a unitary similarity, so a complex factor of any size costs
    what a real one does and no dense matrix is formed."""
    import scipy.linalg as sl
    return sl.eigvalsh_tridiagonal(d, np.abs(e))


@functools.lru_cache(maxsize=None)
def _kron_sum(n1, n2, cplx):
    import scipy.sparse as sp
    bands = [factor_bands(n1, *_T1, cplx, 1), factor_bands(n2, *_T2, cplx, 2)]
    T1, T2 = [sp.diags([np.conj(e), d.astype(C64 if cplx else F64), e], [-1, 0, 1], format="csr") for d, e in bands]
    A = (sp.kron(sp.identity(n2), T1) + sp.kron(T2, sp.identity(n1))).tocsr()
    A.sum_duplicates(); A.sort_indices()
    lam = np.sort(np.add.outer(_tridiag_eigvalsh(*bands[0]), _tridiag_eigvalsh(*bands[1])).ravel())
    ip, ix, d = A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(C64 if cplx else F64)
    for a in (ip, ix, d, lam):
        a.setflags(write=False)
    return ip, ix, d, lam, float(np.max(np.abs(lam)))


def kron_sum(n1, n2, dtype):
    """-> (indptr, indices, data in dtype, the eigenvalues ascending, |A|_2) of I (x) T1 + T2 (x) I, n = n1 n2 rows, sorted CSR.
    A complex dtype takes the complex factors (a Hermitian matrix that is not real)."""
    ip, ix, d, lam, nrm = _kron_sum(n1, n2, np.dtype(dtype).kind == "c")
    return ip, ix, d.astype(dtype), lam, nrm


def csr_double(ip, ix, d, shape=None):
    """The operator in double (complex double) as scipy.sparse, whatever the dtype under test (square unless shape is given)."""
    import scipy.sparse as sp
    return sp.csr_matrix((d.astype(C64 if d.dtype.kind == "c" else F64), ix, ip), shape=shape or (ip.size - 1, ip.size - 1))


def true_residual(A, vals, X):
    """max_i |A x_i - theta_i x_i|_2 in double, A a scipy.sparse matrix in double."""
    Xw = np.asarray(X).astype(C64 if (np.asarray(X).dtype.kind == "c" or A.dtype.kind == "c") else F64)
    return max(float(np.linalg.norm(A @ Xw[i] - float(vals[i]) * Xw[i])) for i in range(len(vals)))


def expm_exact(n1, n2, t, v, cplx):
    """exp(t (I (x) T1 + T2 (x) I)) v in double (complex double) from the factors' dense exponentials."""
    import scipy.linalg as sl
    T1, T2 = factors(n1, n2, cplx)
    E1, E2 = sl.expm(t * T1), sl.expm(t * T2)
    V = np.asarray(v).astype(C64 if (cplx or np.asarray(v).dtype.kind == "c") else F64).reshape(n2, n1)
    return (E2 @ V @ E1.T).reshape(-1)


# ---------------------------------------------------------------------------------------------- sizes past the kernels' caps
TILE_ROWS = {"float64": 128, "complex128": 64, "float32": 256, "complex64": 128}      # 64 packs of 16 bytes


def rotate_grid(num_cu, me, q, coef_bytes):
    """launch_lz_rotate's rule (csrc/eigsh_fuse.hpp): me KiB of tile and the me x qp coefficient block in LDS (qp = q rounded up
    to CB = 2 for q <= 8, else 4), per_cu = clamp(160 KiB / lds, 1, 8) workgroups a CU -> (the cap on the grid, per_cu)."""
    cb = 2 if q <= 8 else 4
    qp = (q + cb - 1) // cb * cb
    lds = me * 64 * 16 + me * qp * coef_bytes
    per_cu = max(1, min(8, (160 << 10) // lds))
    return num_cu * per_cu, per_cu


def n2_for_tiles(n1, rows, tiles):
    """The least n2 for which n1 n2 rows make more than `tiles` whole tiles of `rows` rows and a partial last one."""
    n2 = (tiles * rows) // n1 + 1
    while (n1 * n2) % rows == 0:
        n2 += 1
    return n2


# ---------------------------------------------------------------------------------------------- the product, for Svds
def rect_bands(rows, cols, tops, lo, hi, off, cplx, seed):
    """-> (d, e): the rows x cols factor has B_ii = d_i for i < r = min(rows, cols) and B_{i, i+1} = e_i for i < min(r, cols - 1);
    d = linspace(lo, hi, r) shuffled by default_rng(seed) with isolated large entries `tops` spread through it as in
    factor_bands, e_i = off (real) or off exp(1j i) (complex)."""
    r = min(rows, cols)
    d = np.linspace(lo, hi, r)
    np.random.default_rng(seed).shuffle(d)
    d[np.linspace(0, r - 1, len(tops) + 2).astype(int)[1:-1]] = tops
    j = np.arange(min(r, cols - 1))
    return d, (off * np.exp(1j * j) if cplx else np.full(j.size, float(off)))


def _rect_csr(rows, cols, d, e, cplx):
    import scipy.sparse as sp
    i, j = np.arange(d.size), np.arange(e.size)
    return sp.csr_matrix((np.concatenate([d.astype(C64 if cplx else F64), e]), (np.concatenate([i, j]), np.concatenate([i, j + 1]))), shape=(rows, cols))


def _rect_svdvals(rows, cols, d, e):
    """The singular values of the factor, descending, as the square roots of the eigenvalues of the Hermitian tridiagonal B^H B
    (rows >= cols) or B B^H (wide), through _tridiag_eigvalsh: no dense matrix whatever the factor's size."""
    if rows >= cols:
        diag = d * d + np.concatenate([[0.0], np.abs(e) ** 2])[:d.size]
        off = d[:e.size] * e
    else:
        diag = d * d + np.abs(e) ** 2
        off = e[:d.size - 1] * d[1:]
    return np.sqrt(np.maximum(_tridiag_eigvalsh(diag, off), 0.0))[::-1]


@functools.lru_cache(maxsize=None)
def _kron_product(r1, c1, r2, c2, cplx):
    import scipy.sparse as sp
    b1 = rect_bands(r1, c1, [2.0, 1.5], .5, .6, .02, cplx, 3)
    b2 = rect_bands(r2, c2, [3.0, 2.2, 1.6], .7, 1.0, .03, cplx, 4)
    B = sp.kron(_rect_csr(r2, c2, *b2, cplx), _rect_csr(r1, c1, *b1, cplx)).tocsr()
    B.sum_duplicates(); B.sort_indices()
    s = np.sort(np.outer(_rect_svdvals(r1, c1, *b1), _rect_svdvals(r2, c2, *b2)).ravel())[::-1].copy()
    ip, ix, d = B.indptr.astype(np.int32), B.indices.astype(np.int32), B.data.astype(C64 if cplx else F64)
    for a in (ip, ix, d, s):
        a.setflags(write=False)
    return ip, ix, d, s, (r1 * r2, c1 * c2)


def kron_product(r1, c1, r2, c2, dtype):
    """-> (indptr, indices, data in dtype, the min(r1, c1) min(r2, c2) non-trivial singular values descending, (M, N)) of
    B2 (x) B1, B1 r1 x c1 and B2 r2 x c2 (rect_bands; isolated singular values 2, 1.5 over [.5, .6] and 3, 2.2, 1.6 over [.7, 1])."""
    ip, ix, d, s, shape = _kron_product(r1, c1, r2, c2, np.dtype(dtype).kind == "c")
    return ip, ix, d.astype(dtype), s, shape
