// Block-Jacobi: M = blockdiag(A_bb)^-1, the diagonal blocks of A (1 .. 32 rows each: the unknowns of a grid node, or a grid line)
// inverted on the device at creation and kept densely.  No reference analogue; the arithmetic is the statement in the header
// (sprs_bjacobi_*), the layout is bjacobi_plan.hpp, DESIGN.md §4r.
//
//  * Inversion (set-up, bj_invert_kernel).  A block is worked by a GROUP of lanes inside one wavefront, lane i owning row i of
//    the augmented [W | V] in LDS (stored column-major per group, so the lanes of a group touch neighbouring words): it gathers
//    its row of the block from row s_b + i of A, and in step k of the Gauss-Jordan elimination every lane finds the pivot row
//    by reading the magnitudes of column k in ascending row — the same loop in every lane, so all agree on p without a vote —
//    lane j scales column j of row p, and lane i != p eliminates its row.  Every element receives its updates in the order of
//    k, as the statement fixes: the lane mapping does not show in the bits.  A group's LDS traffic is ordered by
//    wave_lds_fence(), never by __syncthreads(); the groups of a workgroup share nothing, no workgroup waits for another and
//    every loop is bounded by m.  The blocks are binned by size (<= 4, <= 8, <= 16, <= 32), one launch per non-empty bin, LDS
//    sized per bin; row k of the inverse, V[perm[k]], goes straight into the packed layout.  The first singular block is an
//    atomicMin on a device word.
//  * Application (the hot path, bj_apply_kernel).  One launch; a wavefront takes a slice of the layout, grid-striding over the
//    slices under the context's `grid` knob.  Each lane loads the `in` entry of its row (a scalar load: the vectors need the
//    alignment of one element only) and puts it in the wavefront's own 64-entry LDS region; then it folds its row of the
//    inverse, j ascending, matrix entries by coalesced wavefront loads and the block's `in` values from LDS (lanes of one block
//    read the same word: a broadcast), and stores its `out` entry.
//    in == out is safe: a wavefront reads all the `in` entries of its rows before it writes any `out` entry, and no block
//    crosses a wavefront, so no entry another wavefront still has to read is ever overwritten.
#include <limits>

#include "device.hpp"
#include "bjacobi_plan.hpp"

using namespace sprs;

namespace {

constexpr int BJ_BINS = 4;
constexpr int BJ_BIN_MAX[BJ_BINS] = {4, 8, 16, BJ_MAX_BLOCK};
static_assert(BJ_MAX_BLOCK == SPRS_BJACOBI_MAX_BLOCK, "the plan's cap is the header's");

// mag(a) of the statement: |re a| + |im a|, one addition; |a| for the real types
template <class T> __device__ __forceinline__ Real<T> bj_mag(T a) {
    if constexpr (is_complex<T>::value) return fabs(a.re) + fabs(a.im);
    else return fabs(a);
}

// One group of M lanes per block of `blocks` (blocks of at most M rows), GROUPS groups per workgroup.
template <class T, int M, int GROUPS>
__global__ __launch_bounds__(M * GROUPS) void bj_invert_kernel(int count, const int32_t *__restrict__ blocks, const int32_t *__restrict__ bptr,
                                                               const int32_t *__restrict__ bpos, const int64_t *__restrict__ sbase,
                                                               const int32_t *__restrict__ a_rp, const int32_t *__restrict__ a_ci,
                                                               const T *__restrict__ a_v, T *__restrict__ minv, int *__restrict__ bad) {
    static_assert(M <= WAVE && WAVE % M == 0, "a block's group lives inside one wavefront, one lane per row");
    using R = Real<T>;
    __shared__ T s_w[GROUPS][M * M];     // W and V of the group's block, entry (i, j) at j * M + i
    __shared__ T s_v[GROUPS][M * M];
    const int grp = (int)threadIdx.x / M, i = (int)threadIdx.x % M;
    const int slot = (int)blockIdx.x * GROUPS + grp;
    if (slot >= count) return;           // (the whole group: no barrier below spans groups)
    const int b = blocks[slot];
    const int s = bptr[b], e = bptr[b + 1], m = e - s;   // 1 <= m <= M: creation checked both
    T *w = s_w[grp], *v = s_v[grp];
    const bool own = i < m;
    // ---- the local matrix: W[i][j] = a(s + i, s + j), +0 where it is not stored; V = I
    if (own) {
        for (int j = 0; j < m; ++j) { w[j * M + i] = szero<T>(); v[j * M + i] = j == i ? sone<T>() : szero<T>(); }
        for (int k = a_rp[s + i], ke = a_rp[s + i + 1]; k < ke; ++k) {
            const int c = a_ci[k];
            if (c >= e) break;
            if (c >= s) w[(c - s) * M + i] = a_v[k];
        }
    }
    wave_lds_fence();
    // ---- Gauss-Jordan with implicit row pivoting
    unsigned used = 0;
    int perm = 0;
    bool fail = false;
    for (int k = 0; k < m; ++k) {
        int p = -1;
        R best = R(0);
        for (int r = 0; r < m; ++r) {    // ascending, the same in every lane
            if (used >> r & 1u) continue;
            const R g = bj_mag<T>(w[k * M + r]);
            if (p < 0 || g > best) { p = r; best = g; }
        }
        if (!(best > R(0)) || !(best <= std::numeric_limits<R>::max())) { fail = true; break; }
        used |= 1u << p;
        if (i == k) perm = p;
        const T piv = w[k * M + p];
        wave_lds_fence();                // every lane has read the pivot before lane k overwrites it
        if (own) {                       // lane j scales column j of row p
            w[i * M + p] = sdiv(w[i * M + p], piv);
            v[i * M + p] = sdiv(v[i * M + p], piv);
        }
        wave_lds_fence();
        if (own && i != p) {
            const T f = w[k * M + i];
            for (int j = 0; j < m; ++j) {
                w[j * M + i] = ssub(w[j * M + i], smul(f, w[j * M + p]));
                v[j * M + i] = ssub(v[j * M + i], smul(f, v[j * M + p]));
            }
        }
        wave_lds_fence();
    }
    if (fail) {
        if (i == 0) atomicMin(bad, s);
        return;
    }
    // ---- row i of the inverse is V[perm[i]]: straight into the packed layout
    if (own) {
        const int64_t pos = (int64_t)bpos[b] + i;
        T *dst = minv + sbase[pos / BJ_SLICE] + pos % BJ_SLICE;
        for (int j = 0; j < m; ++j) dst[(int64_t)j * BJ_SLICE] = v[j * M + perm];
    }
}

template <class T, int M, int GROUPS>
void launch_invert(sprs_ctx *c, int count, const int32_t *blocks, const int32_t *bptr, const int32_t *bpos, const int64_t *sbase, const sprs_csr *A,
                   T *minv, int *bad) {
    hipLaunchKernelGGL((bj_invert_kernel<T, M, GROUPS>), dim3((count + GROUPS - 1) / GROUPS), dim3(M * GROUPS), 0, c->stream, count, blocks, bptr, bpos,
                       sbase, A->row_ptr, A->col_idx, (const T *)A->val, minv, bad);
}

// out = M in: a wavefront per slice.  `in` and `out` may be the same vector (the file's header says why that is safe).
template <class T>
__global__ __launch_bounds__(BLOCK) void bj_apply_kernel(int nslice, BjacobiDev<T> P, const T *in, T *out) {
    constexpr int WAVES = BLOCK / WAVE;
    __shared__ T s_x[WAVES][WAVE];
    const int lane = (int)threadIdx.x % WAVE, wv = (int)threadIdx.x / WAVE;
    T *xs = s_x[wv];
    for (int s = (int)blockIdx.x * WAVES + wv; s < nslice; s += (int)gridDim.x * WAVES) {
        const int row0 = P.srow[s];
        const bool has = lane < P.scnt[s];
        const unsigned code = P.code[(size_t)s * BJ_SLICE + lane];
        const int first = (int)(code & 0xffu), m = (int)(code >> 8);       // m = 0 where the lane holds no row
        xs[lane] = has ? in[(size_t)row0 + lane] : szero<T>();
        wave_lds_fence();
        const T *mv = P.minv + P.sbase[s] + lane;
        const T *xb = xs + first;
        T acc = szero<T>();
        // Four matrix loads in flight, folded in order: whole steps of four without a predicate, then ONE step whose loads past
        // the row's end are switched off — a row of 3 (or the last 3 of 7) still has its loads in flight together, where a scalar
        // remainder loop waits for each in turn, and the long rows pay for no predicates.
        int j = 0;
        for (; j + 4 <= m; j += 4) {
            T a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = mv[(int64_t)(j + u) * BJ_SLICE];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = sadd(acc, smul(a[u], xb[j + u]));
        }
        if (j < m) {
            T a[3];
#pragma unroll
            for (int u = 0; u < 3; ++u) a[u] = j + u < m ? mv[(int64_t)(j + u) * BJ_SLICE] : szero<T>();
#pragma unroll
            for (int u = 0; u < 3; ++u)
                if (j + u < m) acc = sadd(acc, smul(a[u], xb[j + u]));
        }
        if (has) out[(size_t)row0 + lane] = acc;
        wave_lds_fence();                // the region is rewritten by the next slice
    }
}

}  // namespace

struct sprs_bjacobi {
    sprs_ctx *ctx = nullptr;
    int dtype = 0;
    int64_t n = 0;
    BjacobiPlan plan;                             // host copy: block_ptr, and where sprs_bjacobi_inverse_* finds every entry
    int32_t *srow = nullptr, *scnt = nullptr;     // device, per slice
    int64_t *sbase = nullptr;
    uint16_t *code = nullptr;                     // device, per position
    void *minv = nullptr;                         // device, plan.slots of T
    void *in_tmp = nullptr, *out_tmp = nullptr;   // staging of the host entry points (lazily allocated)
};

namespace {

template <class T>
int bjacobi_create(const sprs_csr *A, const std::vector<int64_t> &bp, sprs_bjacobi **out, int64_t *row_out) {
    sprs_ctx *c = A->ctx;
    auto *P = new sprs_bjacobi();
    P->ctx = c; P->dtype = A->dtype; P->n = A->nrows;
    auto fail = [&](int st) { sprs_bjacobi_destroy(P); return st; };
    P->plan = bjacobi_plan(bp);
    const BjacobiPlan &L = P->plan;
    if (!L.fits) return fail(refuse(c, "sprs_bjacobi", "the layout has more than 2^31 - 1 positions"));
    if (!dev_upload(&P->srow, L.srow.data(), L.srow.size()) || !dev_upload(&P->scnt, L.scnt.data(), L.scnt.size()) ||
        !dev_upload(&P->sbase, L.sbase.data(), L.sbase.size()) || !dev_upload(&P->code, L.code.data(), L.code.size()))
        return fail(SPRS_ERR_HIP);
    if (hipMalloc(&P->minv, sizeof(T) * ((size_t)L.slots + 2)) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (hipMemsetAsync(P->minv, 0, sizeof(T) * ((size_t)L.slots + 2), c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
    // ---- the bins, and what the inversion reads per block
    std::vector<int32_t> bin_blocks[BJ_BINS], bptr(bp.begin(), bp.end());
    for (int64_t b = 0; b < L.nblocks; ++b) {
        const int64_t m = bp[(size_t)b + 1] - bp[(size_t)b];
        int k = 0;
        while (m > BJ_BIN_MAX[k]) ++k;
        bin_blocks[k].push_back((int32_t)b);
    }
    DevBufs tmp;
    auto run = [&]() -> int {
        int32_t *d_bptr, *d_bpos;
        int *bad;
        int h_bad = INT32_MAX;
        SPRS_TRY(tmp.alloc(c, &d_bptr, bptr.size()));
        SPRS_TRY(tmp.alloc(c, &d_bpos, L.bpos.size()));
        SPRS_TRY(tmp.alloc(c, &bad, 1));
        SPRS_HIP_TRY(c, hipMemcpyAsync(d_bptr, bptr.data(), sizeof(int32_t) * bptr.size(), hipMemcpyHostToDevice, c->stream));
        if (L.nblocks) SPRS_HIP_TRY(c, hipMemcpyAsync(d_bpos, L.bpos.data(), sizeof(int32_t) * L.bpos.size(), hipMemcpyHostToDevice, c->stream));
        SPRS_HIP_TRY(c, hipMemcpyAsync(bad, &h_bad, sizeof(int), hipMemcpyHostToDevice, c->stream));
        T *minv = (T *)P->minv;
        for (int k = 0; k < BJ_BINS; ++k) {
            const int cnt = (int)bin_blocks[k].size();
            if (!cnt) continue;
            int32_t *d_blocks;
            SPRS_TRY(tmp.alloc(c, &d_blocks, (size_t)cnt));
            SPRS_HIP_TRY(c, hipMemcpyAsync(d_blocks, bin_blocks[k].data(), sizeof(int32_t) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
            // groups of 4, 8, 16 and 32 lanes; LDS per workgroup, c64: 64 x 0.5 KB, 16 x 2 KB, 4 x 8 KB, 1 x 32 KB (f64 / c32: 2 x 16 KB)
            if (k == 0) launch_invert<T, 4, 64>(c, cnt, d_blocks, d_bptr, d_bpos, P->sbase, A, minv, bad);
            else if (k == 1) launch_invert<T, 8, 16>(c, cnt, d_blocks, d_bptr, d_bpos, P->sbase, A, minv, bad);
            else if (k == 2) launch_invert<T, 16, 4>(c, cnt, d_blocks, d_bptr, d_bpos, P->sbase, A, minv, bad);
            else if constexpr (sizeof(T) <= 8) launch_invert<T, 32, 2>(c, cnt, d_blocks, d_bptr, d_bpos, P->sbase, A, minv, bad);
            else launch_invert<T, 32, 1>(c, cnt, d_blocks, d_bptr, d_bpos, P->sbase, A, minv, bad);
            SPRS_HIP_TRY(c, hipGetLastError());
        }
        SPRS_HIP_TRY(c, hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));       // (the bins' host lists are read until here)
        if (h_bad != INT32_MAX) { if (row_out) *row_out = h_bad; return SPRS_INVALID_PRECOND; }
        return SPRS_OK;
    };
    const int st = run();
    if (st != SPRS_OK) return fail(st);
    *out = P;
    return SPRS_OK;
}

template <class T>
int bjacobi_mul_host(const sprs_bjacobi *Pc, const T *in, size_t in_len, T *out, size_t out_len) {
    if (!Pc || !in || !out || Pc->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    if (in_len != (size_t)Pc->n || out_len != (size_t)Pc->n) return SPRS_DIM_MISMATCH;
    return staged_apply<T>(Pc, in, out, [&](const T *din, T *dout) { return bjacobi_apply<T>(Pc, din, dout); });
}

// every inverse block, row-major, one after another
template <class T>
int bjacobi_inverse(const sprs_bjacobi *P, T *out, size_t len) {
    if (!P || !out || P->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    const BjacobiPlan &L = P->plan;
    size_t want = 0;
    for (int64_t b = 0; b < L.nblocks; ++b) { const size_t m = (size_t)(L.block_ptr[(size_t)b + 1] - L.block_ptr[(size_t)b]); want += m * m; }
    if (len != want) return SPRS_DIM_MISMATCH;
    sprs_ctx *c = P->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    std::vector<T> packed((size_t)L.slots);
    if (L.slots) SPRS_HIP_TRY(c, hipMemcpyAsync(packed.data(), P->minv, sizeof(T) * packed.size(), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    size_t o = 0;
    for (int64_t b = 0; b < L.nblocks; ++b) {
        const int m = (int)(L.block_ptr[(size_t)b + 1] - L.block_ptr[(size_t)b]);
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) out[o++] = packed[(size_t)L.slot(b, i, j)];
    }
    return SPRS_OK;
}

}  // namespace

namespace sprs {

int bjacobi_check(const sprs_bjacobi *P, const sprs_csr *A, int dtype, size_t n) { return applied_check(P, A, dtype, n); }

template <class T>
int bjacobi_apply(const sprs_bjacobi *P, const T *in, T *out) {
    if (!P || !in || !out || P->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = P->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    const int nslice = (int)P->plan.nslice();
    if (!nslice) return SPRS_OK;
    constexpr int WAVES = BLOCK / WAVE;
    const BjacobiDev<T> D{P->srow, P->scnt, P->sbase, P->code, (const T *)P->minv};
    hipLaunchKernelGGL(bj_apply_kernel<T>, dim3(balanced_grid(c, (nslice + WAVES - 1) / WAVES)), dim3(BLOCK), 0, c->stream, nslice, D, in, out);
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}
template int bjacobi_apply<double>(const sprs_bjacobi *, const double *, double *);
template int bjacobi_apply<cplx>(const sprs_bjacobi *, const cplx *, cplx *);
template int bjacobi_apply<float>(const sprs_bjacobi *, const float *, float *);
template int bjacobi_apply<cplxf>(const sprs_bjacobi *, const cplxf *, cplxf *);

template <class T>
AppliedPrec<T> bjacobi_prec(const sprs_bjacobi *P) {
    return AppliedPrec<T>{P, [](const void *h, const sprs_csr *A, int dtype, size_t n) { return bjacobi_check((const sprs_bjacobi *)h, A, dtype, n); },
                          [](const void *h, const T *in, T *out) { return bjacobi_apply<T>((const sprs_bjacobi *)h, in, out); }};
}
template AppliedPrec<double> bjacobi_prec<double>(const sprs_bjacobi *);
template AppliedPrec<cplx> bjacobi_prec<cplx>(const sprs_bjacobi *);
template AppliedPrec<float> bjacobi_prec<float>(const sprs_bjacobi *);
template AppliedPrec<cplxf> bjacobi_prec<cplxf>(const sprs_bjacobi *);

}  // namespace sprs

#define SPRS_G(...) try { __VA_ARGS__ } catch (...) { return SPRS_ERR_HIP; }

extern "C" {

int sprs_bjacobi_create(const sprs_csr *A, int64_t block_size, const int64_t *block_ptr, int64_t nblocks, sprs_bjacobi **out, int64_t *row_out) {
    SPRS_G(
        if (!A || !out) return SPRS_INVALID_ARGUMENT;
        *out = nullptr;
        if (row_out) *row_out = -1;
        SPRS_TRY(single_gpu_only(A, "sprs_bjacobi"));   // (before the shape: a row block with a halo has more columns than rows)
        if (A->nrows != A->ncols) return SPRS_NOT_SQUARE;
        sprs_ctx *c = A->ctx;
        if ((block_size > 0) == (block_ptr != nullptr))
            return refuse(c, "sprs_bjacobi", "exactly one of block_size > 0 and block_ptr must be given (block_size = %lld, block_ptr %s)",
                          (long long)block_size, block_ptr ? "given" : "null");
        std::vector<int64_t> bp;
        int64_t at = -1;
        switch (bjacobi_block_ptr(A->nrows, block_size, block_ptr, nblocks, bp, &at)) {
            case 0: break;
            case 1: return refuse(c, "sprs_bjacobi", "block_ptr must start at 0 (and nblocks must not be negative)");
            case 2: return refuse(c, "sprs_bjacobi", "block_ptr does not increase strictly at block %lld", (long long)at);
            case 3: return refuse(c, "sprs_bjacobi", "block_ptr must end at the %lld rows of the matrix", (long long)A->nrows);
            default: return refuse(c, "sprs_bjacobi", "block %lld has more than SPRS_BJACOBI_MAX_BLOCK = %d rows", (long long)at, SPRS_BJACOBI_MAX_BLOCK);
        }
        CtxLock lock(c);
        SPRS_HIP_TRY(c, hipSetDevice(c->device));
        SPRS_TRY(sorted_columns_dev(A, "sprs_bjacobi"));
        switch (A->dtype) {
            case DT_D: return bjacobi_create<double>(A, bp, out, row_out);
            case DT_Z: return bjacobi_create<cplx>(A, bp, out, row_out);
            case DT_S: return bjacobi_create<float>(A, bp, out, row_out);
            case DT_C: return bjacobi_create<cplxf>(A, bp, out, row_out);
        }
        return SPRS_INVALID_ARGUMENT;)
}

int sprs_bjacobi_destroy(sprs_bjacobi *P) {
    if (!P) return SPRS_OK;
    if (P->ctx) { (void)hipSetDevice(P->ctx->device); (void)hipStreamSynchronize(P->ctx->stream); }
    for (void *p : {(void *)P->srow, (void *)P->scnt, (void *)P->sbase, (void *)P->code, P->minv, P->in_tmp, P->out_tmp}) if (p) (void)hipFree(p);
    delete P;
    return SPRS_OK;
}

int sprs_bjacobi_info(const sprs_bjacobi *P, int64_t *n, int64_t *nblocks, int64_t *max_block, int64_t *slots) {
    if (!P) return SPRS_INVALID_ARGUMENT;
    if (n) *n = P->n;
    if (nblocks) *nblocks = P->plan.nblocks;
    if (max_block) *max_block = P->plan.max_block;
    if (slots) *slots = P->plan.slots;
    return SPRS_OK;
}

int sprs_bjacobi_block_ptr(const sprs_bjacobi *P, int64_t *block_ptr_out) {
    if (!P || !block_ptr_out) return SPRS_INVALID_ARGUMENT;
    std::copy(P->plan.block_ptr.begin(), P->plan.block_ptr.end(), block_ptr_out);
    return SPRS_OK;
}

#define SPRS_BJACOBI_API(X, T, CT)                                                                                      \
    int sprs_bjacobi_inverse_##X(const sprs_bjacobi *P, CT *out, size_t len) {                                          \
        SPRS_G(return bjacobi_inverse<T>(P, (T *)out, len);)                                                            \
    }                                                                                                                   \
    int sprs_bjacobi_mul_vec_dev_##X(const sprs_bjacobi *P, const CT *in, CT *out) {                                    \
        SPRS_G(return bjacobi_apply<T>(P, (const T *)in, (T *)out);)                                                    \
    }                                                                                                                   \
    int sprs_bjacobi_mul_vec_##X(const sprs_bjacobi *P, const CT *in, size_t il, CT *out, size_t ol) {                  \
        SPRS_G(return bjacobi_mul_host<T>(P, (const T *)in, il, (T *)out, ol);)                                         \
    }
SPRS_BJACOBI_API(d, double, double)
SPRS_BJACOBI_API(z, cplx, sprs_c64)
SPRS_BJACOBI_API(s, float, float)
SPRS_BJACOBI_API(c, cplxf, sprs_c32)

}  // extern "C"
