// CSR SpMM for gfx950: Y = A X for a block of k <= 8 vectors, X and Y row-major n x k (the k values of a row are contiguous).
//
// One pass over the plain CSR arrays serves all k columns: col_idx and val are loaded once per entry, the gather fetches
// the k values of row `col` in one or more 16-byte loads.  With k right-hand sides a 7-point f64 row moves 16 + 88 / k
// bytes per right-hand side instead of 104.
//  * Stream blocks (the row blocks of spmv_kernel, rows of <= LONG_ROW entries): one LANE per row with K accumulators, K a
//    template parameter in {1, 2, 4, 8}.  Every column is folded as spmv_kernel folds it — products x[col] * val added
//    left to right starting from +0.0, one rounding per operation — so column c of Y is bit-identical to the SpMV of
//    column c of X.
//  * Vector blocks (one row longer than LONG_ROW): the wavefront strides the row as spmv_kernel does, each lane folds its
//    entries per column, then the same 64-lane butterfly per column: again the bits of the SpMV.
//  * The walk over the row-block descriptors (wavefront per block, XCD-chunked for cache-resident matrices) is spmv_kernel's.
//  * VEC: the leading dimension equals K and the bases are aligned, so a row of X / Y is min(16, K * sizeof(T))-byte
//    packs.  Otherwise the columns are accessed element-wise under the mask c < k.
//  * DOT (dot_mode 1): per-column partials of conj(u_c).y_c, laid out [column][workgroup] (stride = the grid).
//  * `running` (may be null): a word that counts the columns a batched solve still iterates on; the launch returns at its
//    first instruction once it is zero.
#include "device.hpp"

namespace sprs {

namespace {

template <class T, int K> struct spmm_pack { static constexpr int value = (K * sizeof(T) >= 16) ? (int)(16 / sizeof(T)) : K; };

// the K values of row `row` of a row-major block with leading dimension ld
template <class T, int K, bool VEC>
__device__ __forceinline__ void load_row(const T *__restrict__ base, int64_t row, int ld, int k, T (&out)[K]) {
    if constexpr (VEC) {
        constexpr int CH = spmm_pack<T, K>::value;
        const Pack<T, CH> *p = reinterpret_cast<const Pack<T, CH> *>(base + row * K);
#pragma unroll
        for (int q = 0; q < K / CH; ++q) {
            const Pack<T, CH> v = p[q];
#pragma unroll
            for (int e = 0; e < CH; ++e) out[q * CH + e] = v.v[e];
        }
    } else {
#pragma unroll
        for (int c = 0; c < K; ++c) out[c] = c < k ? base[row * ld + c] : szero<T>();
    }
}
template <class T, int K, bool VEC>
__device__ __forceinline__ void store_row(T *__restrict__ base, int64_t row, int ld, int k, const T (&in)[K]) {
    if constexpr (VEC) {
        constexpr int CH = spmm_pack<T, K>::value;
        Pack<T, CH> *p = reinterpret_cast<Pack<T, CH> *>(base + row * K);
#pragma unroll
        for (int q = 0; q < K / CH; ++q) {
            Pack<T, CH> v;
#pragma unroll
            for (int e = 0; e < CH; ++e) v.v[e] = in[q * CH + e];
            p[q] = v;
        }
    } else {
#pragma unroll
        for (int c = 0; c < K; ++c)
            if (c < k) base[row * ld + c] = in[c];
    }
}

template <class T, int K, bool DOT, bool VEC>
__global__ __launch_bounds__(BLOCK) void spmm_kernel(int n_rowblk, int xcd_chunk, const BlkDesc *__restrict__ desc,
                                                     const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ col_idx,
                                                     const T *__restrict__ val, const T *__restrict__ x, T *__restrict__ y, int ld, int k,
                                                     const T *__restrict__ u, T *__restrict__ part, const int *__restrict__ running) {
    if (running != nullptr && *running == 0) return;             // uniform over the grid; nothing has been stored
    __shared__ T red[NWAVE];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid >> 6;
    T dt[K];
#pragma unroll
    for (int c = 0; c < K; ++c) dt[c] = szero<T>();

    int b, bstep, bend;                                          // spmv_kernel's walk
    if (xcd_chunk) {
        const int chunk = (n_rowblk + 7) >> 3;
        const int xcd = blockIdx.x & 7;
        b = xcd * chunk + (blockIdx.x >> 3) * NWAVE + wv;
        bstep = (gridDim.x >> 3) * NWAVE;
        bend = min(n_rowblk, (xcd + 1) * chunk);
    } else {
        b = blockIdx.x * NWAVE + wv; bstep = gridDim.x * NWAVE; bend = n_rowblk;
    }
    for (; b < bend; b += bstep) {
        const BlkDesc d = desc[b];
        const int ra = d.ra, rb = d.rb & 0x7fffffff;
        if (d.rb >= 0) {
            // ---------------- stream block: one lane per row, K accumulators
            const int r = ra + lane;
            if (r < rb) {
                const int s = row_ptr[r], e = row_ptr[r + 1];
                T acc[K];
#pragma unroll
                for (int c = 0; c < K; ++c) acc[c] = szero<T>();     // mat.rs:103  fold(T::zero(), ..)
                int j = s;
                for (; j + 1 < e; j += 2) {                          // two entries' loads in flight; added in order
                    const int c0 = col_idx[j], c1 = col_idx[j + 1];
                    const T v0 = val[j], v1 = val[j + 1];
                    T x0[K], x1[K];
                    load_row<T, K, VEC>(x, c0, ld, k, x0);
                    load_row<T, K, VEC>(x, c1, ld, k, x1);
#pragma unroll
                    for (int c = 0; c < K; ++c) acc[c] = sadd(acc[c], smul(x0[c], v0));   // mat.rs:104  acc + x[col] * val
#pragma unroll
                    for (int c = 0; c < K; ++c) acc[c] = sadd(acc[c], smul(x1[c], v1));
                }
                if (j < e) {
                    const int c0 = col_idx[j];
                    const T v0 = val[j];
                    T x0[K];
                    load_row<T, K, VEC>(x, c0, ld, k, x0);
#pragma unroll
                    for (int c = 0; c < K; ++c) acc[c] = sadd(acc[c], smul(x0[c], v0));
                }
                store_row<T, K, VEC>(y, r, ld, k, acc);
                if constexpr (DOT) {
                    T uu[K];
                    load_row<T, K, VEC>(u, r, ld, k, uu);
#pragma unroll
                    for (int c = 0; c < K; ++c) dt[c] = sadd(dt[c], smul(sconj(uu[c]), acc[c]));
                }
            }
        } else {
            // ---------------- vector block: this wavefront strides one long row (spmv_kernel's order per column)
            const int r = ra;
            const int s = row_ptr[r], e = row_ptr[r + 1];
            T acc[K];
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = szero<T>();
            for (int j = s + lane; j < e; j += WAVE) {
                const int cj = col_idx[j];
                const T vj = val[j];
                T xj[K];
                load_row<T, K, VEC>(x, cj, ld, k, xj);
#pragma unroll
                for (int c = 0; c < K; ++c) acc[c] = sadd(acc[c], smul(xj[c], vj));
            }
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = wave_sum(acc[c]);
            if (lane == 0) {
                store_row<T, K, VEC>(y, r, ld, k, acc);
                if constexpr (DOT) {
                    T uu[K];
                    load_row<T, K, VEC>(u, r, ld, k, uu);
#pragma unroll
                    for (int c = 0; c < K; ++c) dt[c] = sadd(dt[c], smul(sconj(uu[c]), acc[c]));
                }
            }
        }
    }
    if constexpr (DOT) {
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const T sum = block_sum(dt[c], red);
            if (tid == 0 && c < k) part[(size_t)c * gridDim.x + blockIdx.x] = sum;
        }
    }
}

template <class T, int K>
int launch_k(const sprs_csr *A, int grid, int xcd_chunk, const T *x, T *y, int ld, int k, bool dot, const T *u, T *part, const int *running) {
    sprs_ctx *c = A->ctx;
    constexpr size_t AL = spmm_pack<T, K>::value * sizeof(T);
    const uintptr_t bases = reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | (dot ? reinterpret_cast<uintptr_t>(u) : 0);
    const bool vec = ld == K && k == K && (bases & (AL - 1)) == 0;
    const BlkDesc *desc = reinterpret_cast<const BlkDesc *>(A->blk_desc);
    const T *v = reinterpret_cast<const T *>(A->val);
    auto go = [&](auto dot_tag, auto vec_tag) {
        hipLaunchKernelGGL((spmm_kernel<T, K, decltype(dot_tag)::value, decltype(vec_tag)::value>), dim3(grid), dim3(BLOCK), 0, c->stream,
                           (int)A->n_rowblk, xcd_chunk, desc, A->row_ptr, A->col_idx, v, x, y, ld, k, u, part, running);
    };
    if (dot) { if (vec) go(std::true_type{}, std::true_type{}); else go(std::true_type{}, std::false_type{}); }
    else { if (vec) go(std::false_type{}, std::true_type{}); else go(std::false_type{}, std::false_type{}); }
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

}  // namespace

// workgroups == partials per column of one SpMM launch on A: four per CU, at least one row block per wavefront, multiple of 8
int spmm_grid(const sprs_csr *A) {
    const sprs_ctx *c = A->ctx;
    int g = c->spmv_grid > 0 ? c->spmv_grid : c->num_cu * 4;
    g = std::min(std::max(g, 8), MAX_GRID / 2) & ~7;
    const int need = std::max(8, ((((int)A->n_rowblk + NWAVE - 1) / NWAVE + 7) / 8) * 8);
    return std::min(g, need);
}

template <class T>
int launch_spmm(const sprs_csr *A, const T *x, T *y, int ld, int k, int dot_mode, const T *u, T *part, const int *running) {
    if (k < 1 || k > 8 || ld < k || (dot_mode != 0 && dot_mode != 1)) return SPRS_INVALID_ARGUMENT;
    if (A->nrows == 0) return SPRS_OK;
    const int grid = spmm_grid(A);
    const int xc = A->ctx->xcd_chunk < 0 ? (is_cache_resident(A) ? 1 : 0) : A->ctx->xcd_chunk;
    const bool dot = dot_mode == 1;
    if (k == 1) return launch_k<T, 1>(A, grid, xc, x, y, ld, k, dot, u, part, running);
    if (k == 2) return launch_k<T, 2>(A, grid, xc, x, y, ld, k, dot, u, part, running);
    if (k <= 4) return launch_k<T, 4>(A, grid, xc, x, y, ld, k, dot, u, part, running);
    return launch_k<T, 8>(A, grid, xc, x, y, ld, k, dot, u, part, running);
}

#define SPRS_INST_SPMM(T) template int launch_spmm<T>(const sprs_csr *, const T *, T *, int, int, int, const T *, T *, const int *);
SPRS_INST_SPMM(double)
SPRS_INST_SPMM(cplx)
SPRS_INST_SPMM(float)
SPRS_INST_SPMM(cplxf)

}  // namespace sprs
