// FSAI: the factorised sparse approximate inverse M = G^H G of a Hermitian positive-definite A, G sparse lower triangular on a
// pattern fixed up front (the lower part of pattern(A) or of pattern(A A)).  No reference analogue; the arithmetic is the
// statement in the header (sprs_fsai_*), DESIGN.md §4k.
//
// Applying M is two ordinary SpMVs, through G and through GH = sprs_csr_adjoint(G, 1): both are handles like any other, so
// each gets whatever stream format, tile plan or chains its creation finds, and the result has the bits of the SpMV's row
// fold.  What is new here is the set-up:
//  * Pattern (device).  One lane per row checks that A's columns ascend strictly.  Power 2 takes the structural product from
//    spgemm_dev on A's own arrays and discards its values.  Row i of G keeps the columns <= i of row i of the pattern: count,
//    rocprim::exclusive_scan, fill.  The pattern never crosses PCIe: the counts go to the host once (n words) for the row
//    cap, the length bins and nnz(G), and the bins' row lists go up.
//  * Rows (device, fsai_rows_kernel).  Row i of G is the conjugate of the last column of C^-H, S = C C^H the m x m matrix
//    A(J_i, J_i): m <= 64 and the rows are independent.  A row is worked by a GROUP of lanes inside one wavefront — 8 or
//    16 lanes for rows of at most 8 or 16 entries, a whole wavefront above — lane p owning row p of S: it gathers s_p0 .. s_pp by
//    a merge of row j_p of A against J_i, computes c_pq in column q of the left-looking Cholesky, and accumulates
//    acc_p += c_qp g_q in the back substitution.  The lower triangle lives in LDS, one region per group (groups of one
//    workgroup share nothing); a group's LDS traffic is ordered by wave_lds_fence(), never by __syncthreads().  Every
//    element receives its updates in ascending k (descending q in the substitution), as the statement fixes: the lane
//    mapping does not show in the bits.
//  * Bins.  The rows are binned by length (<= 8, <= 16, <= 32, <= 64), one launch per non-empty bin, LDS sized per bin.
// No kernel waits for another workgroup.  The first failing row of each kind is an atomicMin on a device word.
#include <limits>

#include <rocprim/device/device_scan.hpp>

#include "device.hpp"

using namespace sprs;

namespace {

constexpr int FSAI_BINS = 4;
constexpr int FSAI_BIN_MAX[FSAI_BINS] = {8, 16, 32, SPRS_FSAI_MAX_ROW};

// t / r and (-t) / r for a real r: component-wise
template <class T> __device__ __forceinline__ T fs_divr(T t, Real<T> r) {
    if constexpr (is_complex<T>::value) return T{t.re / r, t.im / r};
    else return t / r;
}
// s_pp: the real part only
template <class T> __device__ __forceinline__ T fs_real(T v) { return sfromr<T>(sre(v)); }

// Row i: len[i] = the columns <= i of row i of the pattern P (ascending, so a prefix).  A row whose prefix does not end in i,
// or that stores no a(i, i), is a zero diagonal.
__global__ __launch_bounds__(BLOCK) void fsai_count_kernel(int n, const int32_t *__restrict__ p_rp, const int32_t *__restrict__ p_ci,
                                                           const int32_t *__restrict__ a_rp, const int32_t *__restrict__ a_ci,
                                                           int32_t *__restrict__ len, int *__restrict__ bad) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int b = p_rp[i], e = p_rp[i + 1];
    int k = b;
    while (k < e && p_ci[k] <= i) ++k;
    len[i] = k - b;
    bool diag = k > b && p_ci[k - 1] == i;
    if (diag && a_ci != p_ci) {          // power 2: i in the pattern does not say that a(i, i) is stored
        diag = false;
        for (int q = a_rp[i]; q < a_rp[i + 1] && a_ci[q] <= i; ++q) diag = a_ci[q] == i;
    }
    if (!diag) atomicMin(bad, i);
}

// the lowest row whose columns do not ascend strictly
__global__ __launch_bounds__(BLOCK) void fsai_sorted_kernel(int n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, int *__restrict__ bad) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    for (int k = rp[i] + 1, e = rp[i + 1]; k < e; ++k)
        if (ci[k] <= ci[k - 1]) { atomicMin(bad, i); return; }
}

__global__ __launch_bounds__(BLOCK) void fsai_fill_kernel(int n, const int32_t *__restrict__ p_rp, const int32_t *__restrict__ p_ci,
                                                          const int32_t *__restrict__ g_rp, int32_t *__restrict__ g_ci) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int b = p_rp[i], o = g_rp[i], m = g_rp[i + 1] - o;
    for (int t = 0; t < m; ++t) g_ci[o + t] = p_ci[b + t];
}

// One group of LANES lanes per row of `rows` (rows of at most M <= LANES entries), GROUPS groups per workgroup.
template <class T, int M, int LANES, int GROUPS>
__global__ __launch_bounds__(LANES * GROUPS) void fsai_rows_kernel(int count, const int32_t *__restrict__ rows, const int32_t *__restrict__ a_rp,
                                                                   const int32_t *__restrict__ a_ci, const T *__restrict__ a_v,
                                                                   const int32_t *__restrict__ g_rp, const int32_t *__restrict__ g_ci,
                                                                   T *__restrict__ g_v, int *__restrict__ bad) {
    static_assert(M <= LANES && LANES <= WAVE && WAVE % LANES == 0, "a row's group lives inside one wavefront, one lane per local row");
    using R = Real<T>;
    constexpr int TRI = M * (M + 1) / 2;
    __shared__ T s_tri[GROUPS][TRI];     // the lower triangle of S, then of C: (p, q) at p (p + 1) / 2 + q
    __shared__ T s_g[GROUPS][M];
    __shared__ int32_t s_j[GROUPS][M];
    const int grp = (int)threadIdx.x / LANES, p = (int)threadIdx.x % LANES;
    const int slot = (int)blockIdx.x * GROUPS + grp;
    if (slot >= count) return;           // (the whole group: no barrier below spans groups)
    const int i = rows[slot];
    const int o = g_rp[i], m = g_rp[i + 1] - o;          // 1 <= m <= M: creation checked both
    T *tri = s_tri[grp], *g = s_g[grp];
    int32_t *J = s_j[grp];
    const bool own = p < m;
    T *mine = tri + p * (p + 1) / 2;
    if (own) J[p] = g_ci[o + p];
    wave_lds_fence();
    // ---- the local matrix: s_pq = a(j_p, j_q), q <= p, +0 where it is not stored; the diagonal's real part only
    if (own) {
        for (int q = 0; q <= p; ++q) mine[q] = szero<T>();
        const int jp = J[p];
        int q = 0;
        for (int k = a_rp[jp], ke = a_rp[jp + 1]; k < ke && q <= p;) {
            const int c = a_ci[k], jq = J[q];
            if (c > jp) break;
            if (c == jq) { mine[q] = q == p ? fs_real<T>(a_v[k]) : a_v[k]; ++k; ++q; }
            else if (c < jq) ++k;
            else ++q;
        }
    }
    wave_lds_fence();
    // ---- S = C C^H, column by column; every lane of the group forms d (the same operations), lane p > q forms c_pq
    bool fail = false;
    for (int q = 0; q < m; ++q) {
        const T *rq = tri + q * (q + 1) / 2;
        R d = sre(rq[q]);
        T t = own && p > q ? mine[q] : szero<T>();
        for (int k = 0; k < q; ++k) {
            const T cq = rq[k];
            d = d - ssq(cq);
            if (own && p > q) t = ssub(t, smul(mine[k], sconj(cq)));
        }
        if (!(d > R(0)) || !(d <= std::numeric_limits<R>::max())) { fail = true; break; }
        const R cqq = ssqrt(d);
        wave_lds_fence();                // column q is read by every lane above, written below
        if (p == q) mine[q] = sfromr<T>(cqq);
        else if (own && p > q) mine[q] = fs_divr<T>(t, cqq);
        wave_lds_fence();
    }
    if (fail) {
        if (p == 0) atomicMin(bad, i);
        return;
    }
    // ---- the row of G: g_q from the last to the first, acc_p += c_qp g_q for every p < q as soon as g_q is known
    T acc = szero<T>();
    for (int q = m - 1; q >= 0; --q) {
        if (p == q) {
            const R cqq = sre(mine[q]);
            g[q] = q == m - 1 ? sfromr<T>(R(1) / cqq) : fs_divr<T>(sneg(acc), cqq);
        }
        wave_lds_fence();
        if (p < q) acc = sadd(acc, smul(tri[q * (q + 1) / 2 + p], g[q]));
    }
    if (own) g_v[o + p] = g[p];
}

template <class T, int M, int LANES, int GROUPS>
void launch_rows(sprs_ctx *c, int count, const int32_t *rows, const sprs_csr *A, const int32_t *g_rp, const int32_t *g_ci, T *g_v, int *bad) {
    hipLaunchKernelGGL((fsai_rows_kernel<T, M, LANES, GROUPS>), dim3((count + GROUPS - 1) / GROUPS), dim3(LANES * GROUPS), 0, c->stream, count, rows,
                       A->row_ptr, A->col_idx, (const T *)A->val, g_rp, g_ci, g_v, bad);
}

template <class T> struct create_dev_of;
template <> struct create_dev_of<double> { static int go(sprs_ctx *c, int64_t n, int64_t nnz, const int32_t *rp, const int32_t *ci, const double *v, sprs_csr **o) { return sprs_csr_create_dev_d(c, n, n, nnz, rp, ci, v, 1, o); } };
template <> struct create_dev_of<cplx> { static int go(sprs_ctx *c, int64_t n, int64_t nnz, const int32_t *rp, const int32_t *ci, const cplx *v, sprs_csr **o) { return sprs_csr_create_dev_z(c, n, n, nnz, rp, ci, (const sprs_c64 *)v, 1, o); } };
template <> struct create_dev_of<float> { static int go(sprs_ctx *c, int64_t n, int64_t nnz, const int32_t *rp, const int32_t *ci, const float *v, sprs_csr **o) { return sprs_csr_create_dev_s(c, n, n, nnz, rp, ci, v, 1, o); } };
template <> struct create_dev_of<cplxf> { static int go(sprs_ctx *c, int64_t n, int64_t nnz, const int32_t *rp, const int32_t *ci, const cplxf *v, sprs_csr **o) { return sprs_csr_create_dev_c(c, n, n, nnz, rp, ci, (const sprs_c32 *)v, 1, o); } };

}  // namespace

struct sprs_fsai {
    sprs_ctx *ctx = nullptr;
    int dtype = 0, power = 0;
    int64_t n = 0, nnz = 0, max_row = 0;
    sprs_csr *G = nullptr, *GH = nullptr;         // owned; G owns its three arrays
    void *tbuf = nullptr;                         // device, n of T: G in
    void *in_tmp = nullptr, *out_tmp = nullptr;   // staging of the host entry points (lazily allocated)
};

namespace {

template <class T>
int fsai_create(const sprs_csr *A, int power, sprs_fsai **out, int64_t *row_out) {
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    const int64_t n = A->nrows;
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    // ---- the ascending-columns check, on the device: the pattern never crosses PCIe
    SPRS_TRY(sorted_columns_dev(A, "sprs_fsai"));
    DevBufs tmp;
    int *bad;                            // the lowest row of: [0] a zero diagonal, [1] a pivot that is not positive
    SPRS_TRY(tmp.alloc(c, &bad, 2));
    const int h_none[2] = {INT32_MAX, INT32_MAX};
    int h_bad[2] = {INT32_MAX, INT32_MAX};
    const dim3 rgrid((unsigned)((n + BLOCK - 1) / BLOCK));
    SPRS_HIP_TRY(c, hipMemcpyAsync(bad, h_none, sizeof(h_none), hipMemcpyHostToDevice, c->stream));
    // ---- the pattern P
    const int32_t *p_rp = A->row_ptr, *p_ci = A->col_idx;
    if (power == 2) {
        int32_t *q_rp = nullptr, *q_ci = nullptr;
        T *q_v = nullptr;
        int64_t q_nnz = 0;
        SPRS_TRY(spgemm_dev<T>(c, "sprs_fsai", n, n, n, A->row_ptr, A->col_idx, (const T *)A->val, A->row_ptr, A->col_idx, (const T *)A->val,
                               &q_rp, &q_ci, &q_v, &q_nnz, nullptr));
        tmp.p.push_back(q_rp); tmp.p.push_back(q_ci);
        (void)hipFree(q_v);              // structural: the product's values are not used
        p_rp = q_rp; p_ci = q_ci;
    }
    // ---- count
    int32_t *len, *g_rp;
    SPRS_TRY(tmp.alloc(c, &len, (size_t)n + 1));
    SPRS_TRY(tmp.alloc(c, &g_rp, (size_t)n + 1));
    SPRS_HIP_TRY(c, hipMemsetAsync(len, 0, sizeof(int32_t) * ((size_t)n + 1), c->stream));
    if (n) hipLaunchKernelGGL(fsai_count_kernel, rgrid, dim3(BLOCK), 0, c->stream, (int)n, p_rp, p_ci, A->row_ptr, A->col_idx, len, bad);
    SPRS_HIP_TRY(c, hipGetLastError());
    std::vector<int32_t> h_len((size_t)n);
    if (n) SPRS_HIP_TRY(c, hipMemcpyAsync(h_len.data(), len, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_bad[0] != INT32_MAX) { if (row_out) *row_out = h_bad[0]; return SPRS_ZERO_DIAGONAL; }
    // ---- the cap, the bins and nnz(G) from the counts
    std::vector<int32_t> bin_rows[FSAI_BINS];
    int64_t nnz_g = 0, max_row = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int32_t m = h_len[(size_t)i];
        if (m > SPRS_FSAI_MAX_ROW) {
            snprintf(c->err, sizeof(c->err), "sprs_fsai: row %lld of G has %d entries, more than SPRS_FSAI_MAX_ROW = %d", (long long)i, (int)m, SPRS_FSAI_MAX_ROW);
            return SPRS_INVALID_ARGUMENT;
        }
        int b = 0;
        while (m > FSAI_BIN_MAX[b]) ++b;
        bin_rows[b].push_back((int32_t)i);
        nnz_g += m; max_row = std::max<int64_t>(max_row, m);
    }
    if (nnz_g >= INT32_MAX) return SPRS_INVALID_ARGUMENT;
    // ---- scan, fill
    int32_t *g_ci;
    T *g_v;
    SPRS_TRY(tmp.alloc(c, &g_ci, (size_t)nnz_g));
    SPRS_TRY(tmp.alloc(c, &g_v, (size_t)nnz_g));
    size_t scan_bytes = 0;
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, len, g_rp, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), c->stream));
    char *scratch;
    SPRS_TRY(tmp.alloc(c, &scratch, scan_bytes));
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(scratch, scan_bytes, len, g_rp, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), c->stream));
    if (n) hipLaunchKernelGGL(fsai_fill_kernel, rgrid, dim3(BLOCK), 0, c->stream, (int)n, p_rp, p_ci, g_rp, g_ci);
    SPRS_HIP_TRY(c, hipGetLastError());
    // ---- the rows, one launch per non-empty bin
    int32_t *d_rows[FSAI_BINS] = {nullptr, nullptr, nullptr, nullptr};
    for (int b = 0; b < FSAI_BINS; ++b) {
        const int cnt = (int)bin_rows[b].size();
        if (!cnt) continue;
        SPRS_TRY(tmp.alloc(c, &d_rows[b], (size_t)cnt));
        SPRS_HIP_TRY(c, hipMemcpyAsync(d_rows[b], bin_rows[b].data(), sizeof(int32_t) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
        // groups of 8, 16, 64 and 64 lanes; LDS per workgroup, c64: 32 x 0.7 KB, 16 x 2.5 KB, 4 x 9 KB, 1 x 34 KB
        if (b == 0) launch_rows<T, 8, 8, 32>(c, cnt, d_rows[b], A, g_rp, g_ci, g_v, bad + 1);
        else if (b == 1) launch_rows<T, 16, 16, 16>(c, cnt, d_rows[b], A, g_rp, g_ci, g_v, bad + 1);
        else if (b == 2) launch_rows<T, 32, 64, 4>(c, cnt, d_rows[b], A, g_rp, g_ci, g_v, bad + 1);
        else launch_rows<T, SPRS_FSAI_MAX_ROW, 64, 1>(c, cnt, d_rows[b], A, g_rp, g_ci, g_v, bad + 1);
        SPRS_HIP_TRY(c, hipGetLastError());
    }
    SPRS_HIP_TRY(c, hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));       // (the bins' host lists are read until here)
    if (h_bad[1] != INT32_MAX) { if (row_out) *row_out = h_bad[1]; return SPRS_INVALID_PRECOND; }
    // ---- the two handles and the intermediate vector
    for (void *q : {(void *)len, (void *)scratch, (void *)bad, (void *)d_rows[0], (void *)d_rows[1], (void *)d_rows[2], (void *)d_rows[3]}) if (q) tmp.free(q);
    if (power == 2) { tmp.free(const_cast<int32_t *>(p_rp)); tmp.free(const_cast<int32_t *>(p_ci)); }
    auto *P = new sprs_fsai();
    P->ctx = c; P->dtype = A->dtype; P->power = power; P->n = n; P->nnz = nnz_g; P->max_row = max_row;
    auto fail = [&](int st) { sprs_fsai_destroy(P); return st; };
    int st = create_dev_of<T>::go(c, n, nnz_g, g_rp, g_ci, g_v, &P->G);
    if (st != SPRS_OK) return fail(st);
    P->G->owns_arrays = true;            // adopted, and from here on released with the handle
    tmp.release(g_rp); tmp.release(g_ci); tmp.release(g_v);
    st = sprs_csr_adjoint(P->G, 1, &P->GH);
    if (st != SPRS_OK) return fail(st);
    if (hipMalloc(&P->tbuf, sizeof(T) * ((size_t)n + 2)) != hipSuccess) return fail(SPRS_ERR_HIP);
    *out = P;
    return SPRS_OK;
}

template <class T>
int fsai_mul_host(const sprs_fsai *Pc, const T *in, size_t in_len, T *out, size_t out_len) {
    if (!Pc || !in || !out || Pc->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    if (in_len != (size_t)Pc->n || out_len != (size_t)Pc->n) return SPRS_DIM_MISMATCH;
    return staged_apply<T>(Pc, in, out, [&](const T *din, T *dout) { return fsai_apply<T>(Pc, din, dout); });
}

}  // namespace

namespace sprs {

int fsai_check(const sprs_fsai *P, const sprs_csr *A, int dtype, size_t n) { return applied_check(P, A, dtype, n); }

int sorted_columns_dev(const sprs_csr *A, const char *who) {
    sprs_ctx *c = A->ctx;
    const int64_t n = A->nrows;
    DevBufs tmp;
    int *bad, h_bad = INT32_MAX;
    SPRS_TRY(tmp.alloc(c, &bad, 1));
    SPRS_HIP_TRY(c, hipMemcpyAsync(bad, &h_bad, sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (n) hipLaunchKernelGGL(fsai_sorted_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, (int)n, A->row_ptr, A->col_idx, bad);
    SPRS_HIP_TRY(c, hipGetLastError());
    SPRS_HIP_TRY(c, hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_bad == INT32_MAX) return SPRS_OK;
    snprintf(c->err, sizeof(c->err), "%s: the column indices of row %lld are not strictly ascending", who, (long long)h_bad);
    return SPRS_INVALID_ARGUMENT;
}

template <class T>
int fsai_apply(const sprs_fsai *P, const T *in, T *out) {
    if (!P || !in || !out || P->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = P->ctx;
    CtxLock lock(c);   // tbuf is per-handle scratch
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (!P->n) return SPRS_OK;
    SPRS_TRY(launch_spmv<T>(P->G, SpmvPart::Whole, in, (T *)P->tbuf, 0, nullptr, nullptr, nullptr, nullptr));
    return launch_spmv<T>(P->GH, SpmvPart::Whole, (const T *)P->tbuf, out, 0, nullptr, nullptr, nullptr, nullptr);
}
template int fsai_apply<double>(const sprs_fsai *, const double *, double *);
template int fsai_apply<cplx>(const sprs_fsai *, const cplx *, cplx *);
template int fsai_apply<float>(const sprs_fsai *, const float *, float *);
template int fsai_apply<cplxf>(const sprs_fsai *, const cplxf *, cplxf *);

template <class T>
AppliedPrec<T> fsai_prec(const sprs_fsai *P) {
    return AppliedPrec<T>{P, [](const void *h, const sprs_csr *A, int dtype, size_t n) { return fsai_check((const sprs_fsai *)h, A, dtype, n); },
                          [](const void *h, const T *in, T *out) { return fsai_apply<T>((const sprs_fsai *)h, in, out); }};
}
template AppliedPrec<double> fsai_prec<double>(const sprs_fsai *);
template AppliedPrec<cplx> fsai_prec<cplx>(const sprs_fsai *);
template AppliedPrec<float> fsai_prec<float>(const sprs_fsai *);
template AppliedPrec<cplxf> fsai_prec<cplxf>(const sprs_fsai *);

}  // namespace sprs

#define SPRS_G(...) try { __VA_ARGS__ } catch (...) { return SPRS_ERR_HIP; }

extern "C" {

int sprs_fsai_create(const sprs_csr *A, int power, sprs_fsai **out, int64_t *row_out) {
    SPRS_G(
        if (!A || !out) return SPRS_INVALID_ARGUMENT;
        *out = nullptr;
        if (row_out) *row_out = -1;
        SPRS_TRY(single_gpu_only(A, "sprs_fsai"));   // (before the shape: a row block with a halo has more columns than rows)
        if (power != 1 && power != 2) {
            snprintf(A->ctx->err, sizeof(A->ctx->err), "sprs_fsai: power must be 1 or 2, got %d", power);
            return SPRS_INVALID_ARGUMENT;
        }
        if (A->nrows != A->ncols) return SPRS_NOT_SQUARE;
        switch (A->dtype) {
            case DT_D: return fsai_create<double>(A, power, out, row_out);
            case DT_Z: return fsai_create<cplx>(A, power, out, row_out);
            case DT_S: return fsai_create<float>(A, power, out, row_out);
            case DT_C: return fsai_create<cplxf>(A, power, out, row_out);
        }
        return SPRS_INVALID_ARGUMENT;)
}

int sprs_fsai_destroy(sprs_fsai *P) {
    if (!P) return SPRS_OK;
    if (P->ctx) { (void)hipSetDevice(P->ctx->device); (void)hipStreamSynchronize(P->ctx->stream); }
    sprs_csr_destroy(P->GH); sprs_csr_destroy(P->G);
    for (void *p : {P->tbuf, P->in_tmp, P->out_tmp}) if (p) (void)hipFree(p);
    delete P;
    return SPRS_OK;
}

int sprs_fsai_info(const sprs_fsai *P, int64_t *n, int64_t *nnz_g, int64_t *max_row, int64_t *power) {
    if (!P) return SPRS_INVALID_ARGUMENT;
    if (n) *n = P->n;
    if (nnz_g) *nnz_g = P->nnz;
    if (max_row) *max_row = P->max_row;
    if (power) *power = P->power;
    return SPRS_OK;
}

int sprs_fsai_factor(const sprs_fsai *P, int which, const sprs_csr **out) {
    if (!P || !out || which < 0 || which > 1) return SPRS_INVALID_ARGUMENT;
    *out = which ? P->GH : P->G;
    return SPRS_OK;
}

#define SPRS_FSAI_API(X, T, CT)                                                                                         \
    int sprs_fsai_mul_vec_dev_##X(const sprs_fsai *P, const CT *in, CT *out) {                                          \
        SPRS_G(return fsai_apply<T>(P, (const T *)in, (T *)out);)                                                       \
    }                                                                                                                   \
    int sprs_fsai_mul_vec_##X(const sprs_fsai *P, const CT *in, size_t il, CT *out, size_t ol) {                        \
        SPRS_G(return fsai_mul_host<T>(P, (const T *)in, il, (T *)out, ol);)                                            \
    }
SPRS_FSAI_API(d, double, double)
SPRS_FSAI_API(z, cplx, sprs_c64)
SPRS_FSAI_API(s, float, float)
SPRS_FSAI_API(c, cplxf, sprs_c32)

}  // extern "C"
