// C = A B for two CSR operators, built in HBM (sprs_csr_matmul).  The contract is the serial Gustavson loop of the
// header: row i of C folds, per column j, the products a_ik b_kj in the stored order of A's row i (and, within one k, of B's row
// k) onto an accumulator that starts at +0; the stored pattern is the structural one; the columns of a row ascend.
//
// Every accumulator is updated by plain loads and stores of the ONE lane that holds the pair (k, j): B's rows are strictly
// ascending (checked on the device), so within one k no two lanes meet on a column, and successive k are separated by a
// workgroup barrier.  No floating-point atomic appears; the integer atomics only hand out table slots, whose position never
// reaches the result (each row is sorted by column before it is written).
//
//   bound      u_i = sum over the stored a_ik of nnz(B row k), one lane per row, in 64 bits: an upper bound of the products and
//              so of the distinct columns of row i.  u_i alone deals the row to a path; every table below is sized from its
//              path's largest u_i, so a table can never fill (the probing loops are bounded by the capacity all the same).
//   lists      per path: flag, rocprim::exclusive_scan, fill in ascending row order
//   symbolic   distinct columns per row -> scan -> row_ptr (total checked against 2^31 - 1) -> allocation
//   numeric    the same walk with values; each row's occupied slots sorted by column and written at row_ptr[i]
//
// The three paths:
//   short      u_i <= SPG_SHORT_MAX: eight rows per wavefront, eight lanes and a 64-slot LDS table per row (it may
//              fill to the last slot, never beyond), rank by counting
//   table      u_i <= table_max<T>(): one workgroup per row, an open-addressing (column, accumulator) table in LDS at a load of
//              at most one half, compaction of the occupied slots and a bitonic sort of (column, slot) in LDS
//   fallback   anything larger: a dense accumulator + mark array of B->ncols entries per workgroup in global scratch, the marked
//              columns gathered in ascending order.  At most SPG_FB_GROUPS workgroups, and no more than fit SPG_FB_BYTES of
//              scratch (one workgroup at least): the scratch is max(SPG_FB_BYTES, ncols (sizeof(T) + 4)) bytes at the most.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>

#include "internal.hpp"

using namespace sprs;

namespace {

constexpr int SPG_SHORT_MAX = 64;        // largest u_i of the short path (a 7-point stencil squared: 49)
constexpr int SPG_SHORT_SLOTS = 64;      // its table: as many slots as there can be columns
constexpr int SPG_SUB = 8;               // lanes per row of the short path; WAVE / SPG_SUB rows per wavefront
constexpr int SPG_WAVE = 64;
constexpr int SPG_SHORT_ROWS = SPG_WAVE / SPG_SUB;
constexpr int SPG_FB_GROUPS = 1024;      // most workgroups of the fallback path (four per CU)
constexpr size_t SPG_FB_BYTES = (size_t)256 << 20;

// slots of the table path: 4096 for f32, 2048 for the wider scalars (keys + accumulators + sort keys: 48 KiB of LDS at the most,
// three workgroups per CU); rows of at most half as many products take the path
template <class T> constexpr int table_slots() { return sizeof(T) <= 4 ? 4096 : 2048; }
template <class T> constexpr int table_max() { return table_slots<T>() / 2; }

__device__ __forceinline__ uint32_t spg_hash(int32_t j, int log2_slots) { return ((uint32_t)j * 2654435769u) >> (32 - log2_slots); }

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }

// Claims the slot of column j in an open-addressing table of `slots` keys (-1: free), or finds it: slot index and whether this
// call claimed it; -1 when `slots` probes found neither (cannot happen while the table is sized by the bound).
template <int SLOTS>
__device__ __forceinline__ int spg_slot(int32_t *keys, int32_t j, bool &fresh) {
    uint32_t h = spg_hash(j, ilog2(SLOTS));
    for (int t = 0; t < SLOTS; ++t) {
        const int32_t old = atomicCAS(&keys[h], -1, j);
        if (old == -1 || old == j) { fresh = old == -1; return (int)h; }
        h = (h + 1) & (SLOTS - 1);
    }
    fresh = false;
    return -1;
}

// u_i and the path of every row of A; the smallest row of A with a column outside [0, nrB) goes to bad[0]
__global__ __launch_bounds__(BLOCK) void spg_bound_kernel(int64_t nrA, int64_t nrB, const int32_t *__restrict__ a_rp, const int32_t *__restrict__ a_ci,
                                                          const int32_t *__restrict__ b_rp, int64_t short_max, int64_t tab_max,
                                                          uint8_t *__restrict__ path, int *__restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nrA) return;
    int64_t u = 0;
    for (int32_t p = a_rp[i]; p < a_rp[i + 1]; ++p) {
        const int32_t k = a_ci[p];
        if (k < 0 || (int64_t)k >= nrB) { atomicMin(bad, (int)i); continue; }
        u += (int64_t)(b_rp[k + 1] - b_rp[k]);
    }
    path[i] = u <= short_max ? 0 : u <= tab_max ? 1 : 2;
}

// the smallest row of B whose columns are not strictly ascending inside [0, ncB) goes to bad[1]
__global__ __launch_bounds__(BLOCK) void spg_check_b_kernel(int64_t nrB, int64_t ncB, const int32_t *__restrict__ b_rp, const int32_t *__restrict__ b_ci,
                                                            int *__restrict__ bad) {
    const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r >= nrB) return;
    int64_t prev = -1;
    for (int32_t q = b_rp[r]; q < b_rp[r + 1]; ++q) {
        const int64_t c = b_ci[q];
        if (c <= prev || c >= ncB) { atomicMin(bad + 1, (int)r); break; }
        prev = c;
    }
}

struct IsPath {
    int which;
    __host__ __device__ int32_t operator()(uint8_t p) const { return p == which ? 1 : 0; }
};

__global__ __launch_bounds__(BLOCK) void spg_fill_lists_kernel(int64_t nrA, const uint8_t *__restrict__ path, const int32_t *__restrict__ pos0,
                                                               const int32_t *__restrict__ pos1, const int32_t *__restrict__ pos2,
                                                               int32_t *__restrict__ l0, int32_t *__restrict__ l1, int32_t *__restrict__ l2) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= nrA) return;
    const int p = path[i];
    if (p == 0) l0[pos0[i]] = (int32_t)i;
    else if (p == 1) l1[pos1[i]] = (int32_t)i;
    else l2[pos2[i]] = (int32_t)i;
}

__global__ __launch_bounds__(BLOCK) void spg_narrow_kernel(int64_t n, const int64_t *__restrict__ in, int32_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) out[i] = (int32_t)in[i];
}

struct Operands {
    const int32_t *a_rp, *a_ci, *b_rp, *b_ci;
};

// ---------------------------------------------------------------------------------------------------------------- short path
// One wavefront per workgroup, SPG_SHORT_ROWS rows in it.  The walk over A's entries runs to the longest of the wavefront's rows
// so that the barrier between two entries is reached by every lane.
template <class T, bool NUM>
__global__ __launch_bounds__(SPG_WAVE) void spg_short_kernel(int n_list, const int32_t *__restrict__ list, Operands M, const T *__restrict__ a_v,
                                                             const T *__restrict__ b_v, int32_t *__restrict__ cnt, const int32_t *__restrict__ c_rp,
                                                             int32_t *__restrict__ c_ci, T *__restrict__ c_v, int *__restrict__ bad) {
    __shared__ int32_t keys[SPG_SHORT_ROWS][SPG_SHORT_SLOTS];
    __shared__ T vals[NUM ? SPG_SHORT_ROWS : 1][NUM ? SPG_SHORT_SLOTS : 1];
    const int lane = (int)threadIdx.x, sub = lane / SPG_SUB, sl = lane % SPG_SUB;
    const int64_t li = (int64_t)blockIdx.x * SPG_SHORT_ROWS + sub;
    const int32_t row = li < n_list ? list[li] : -1;
    for (int s = sl; s < SPG_SHORT_SLOTS; s += SPG_SUB) keys[sub][s] = -1;
    const int32_t p0 = row >= 0 ? M.a_rp[row] : 0;
    const int32_t len = row >= 0 ? M.a_rp[row + 1] - p0 : 0;
    int32_t maxlen = len;
    for (int d = SPG_WAVE / 2; d > 0; d >>= 1) maxlen = max(maxlen, __shfl_xor(maxlen, d));
    __syncthreads();
    for (int32_t t = 0; t < maxlen; ++t) {
        if (t < len) {
            const int32_t k = M.a_ci[p0 + t];
            T a = szero<T>();
            if (NUM) a = a_v[p0 + t];
            for (int32_t q = M.b_rp[k] + sl; q < M.b_rp[k + 1]; q += SPG_SUB) {
                bool fresh;
                const int h = spg_slot<SPG_SHORT_SLOTS>(keys[sub], M.b_ci[q], fresh);
                if (h < 0) { atomicMin(bad + 2, 0); continue; }
                if (NUM) vals[sub][h] = sadd(fresh ? szero<T>() : vals[sub][h], smul(a, b_v[q]));
            }
        }
        __syncthreads();
    }
    int mine = 0;
    for (int s = sl; s < SPG_SHORT_SLOTS; s += SPG_SUB) {
        const int32_t key = keys[sub][s];
        if (key < 0) continue;
        ++mine;
        if (NUM) {
            int rank = 0;
            for (int x = 0; x < SPG_SHORT_SLOTS; ++x) { const int32_t o = keys[sub][x]; rank += (o >= 0 && o < key) ? 1 : 0; }
            const int64_t d = (int64_t)c_rp[row] + rank;
            c_ci[d] = key; c_v[d] = vals[sub][s];
        }
    }
    if (!NUM) {
        for (int d = SPG_SUB / 2; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
        if (sl == 0 && row >= 0) cnt[row] = mine;
    }
}

// ---------------------------------------------------------------------------------------------------------------- table path
template <class T, bool NUM>
__global__ __launch_bounds__(BLOCK) void spg_table_kernel(const int32_t *__restrict__ list, Operands M, const T *__restrict__ a_v, const T *__restrict__ b_v,
                                                          int32_t *__restrict__ cnt, const int32_t *__restrict__ c_rp, int32_t *__restrict__ c_ci,
                                                          T *__restrict__ c_v, int *__restrict__ bad) {
    constexpr int SLOTS = table_slots<T>(), CAP = table_max<T>();
    __shared__ int32_t keys[SLOTS];
    __shared__ T vals[NUM ? SLOTS : 1];
    __shared__ unsigned long long srt[NUM ? CAP : 1];
    __shared__ int m;
    const int tid = (int)threadIdx.x;
    const int32_t row = list[blockIdx.x];
    for (int s = tid; s < SLOTS; s += BLOCK) keys[s] = -1;
    if (tid == 0) m = 0;
    __syncthreads();
    const int32_t p1 = M.a_rp[row + 1];
    for (int32_t p = M.a_rp[row]; p < p1; ++p) {            // uniform for the workgroup
        const int32_t k = M.a_ci[p];
        T a = szero<T>();
        if (NUM) a = a_v[p];
        for (int32_t q = M.b_rp[k] + tid; q < M.b_rp[k + 1]; q += BLOCK) {
            bool fresh;
            const int h = spg_slot<SLOTS>(keys, M.b_ci[q], fresh);
            if (h < 0) { atomicMin(bad + 2, 0); continue; }
            if (NUM) vals[h] = sadd(fresh ? szero<T>() : vals[h], smul(a, b_v[q]));
        }
        __syncthreads();
    }
    // the occupied slots (at most CAP: the distinct columns are at most u_i), in whatever order: the sort decides
    for (int s = tid; s < SLOTS; s += BLOCK) {
        const int32_t key = keys[s];
        if (key < 0) continue;
        const int pos = atomicAdd(&m, 1);
        if (NUM && pos < CAP) srt[pos] = ((unsigned long long)(uint32_t)key << 32) | (unsigned long long)s;
    }
    __syncthreads();
    const int count = min(m, CAP);
    if (m > CAP && tid == 0) atomicMin(bad + 2, 0);
    if (!NUM) {
        if (tid == 0) cnt[row] = count;
        return;
    }
    int np2 = 1;
    while (np2 < count) np2 <<= 1;
    for (int x = count + tid; x < np2; x += BLOCK) srt[x] = ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= np2; kk <<= 1)
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            for (int x = tid; x < np2; x += BLOCK) {
                const int y = x ^ jj;
                if (y > x) {
                    const unsigned long long ex = srt[x], ey = srt[y];
                    if ((ex > ey) == ((x & kk) == 0)) { srt[x] = ey; srt[y] = ex; }
                }
            }
            __syncthreads();
        }
    const int64_t base = c_rp[row];
    for (int x = tid; x < count; x += BLOCK) {
        const unsigned long long e = srt[x];
        c_ci[base + x] = (int32_t)(e >> 32);
        c_v[base + x] = vals[(int)(e & 0xffffffffull)];
    }
}

// ---------------------------------------------------------------------------------------------------------------- fallback
// Workgroup g takes rows g, g + G, ... of the list.  mark[j] == row + 1 says that column j belongs to the row at hand (the rows
// of one workgroup ascend, the array is zeroed before each pass), so nothing is cleared between rows.
template <class T, bool NUM>
__global__ __launch_bounds__(BLOCK) void spg_fallback_kernel(int n_list, const int32_t *__restrict__ list, Operands M, const T *__restrict__ a_v,
                                                             const T *__restrict__ b_v, int64_t ncB, uint32_t *__restrict__ mark_all, T *__restrict__ acc_all,
                                                             int32_t *__restrict__ cnt, const int32_t *__restrict__ c_rp, int32_t *__restrict__ c_ci,
                                                             T *__restrict__ c_v) {
    __shared__ int total;
    __shared__ int wtot[BLOCK / SPG_WAVE];
    const int tid = (int)threadIdx.x, lane = tid % SPG_WAVE, wave = tid / SPG_WAVE;
    uint32_t *mark = mark_all + (int64_t)blockIdx.x * ncB;
    T *acc = acc_all + (NUM ? (int64_t)blockIdx.x * ncB : 0);
    for (int li = (int)blockIdx.x; li < n_list; li += (int)gridDim.x) {
        const int32_t row = list[li];
        const uint32_t tag = (uint32_t)row + 1u;
        if (tid == 0) total = 0;
        __syncthreads();
        int mine = 0;
        const int32_t p1 = M.a_rp[row + 1];
        for (int32_t p = M.a_rp[row]; p < p1; ++p) {
            const int32_t k = M.a_ci[p];
            T a = szero<T>();
            if (NUM) a = a_v[p];
            for (int32_t q = M.b_rp[k] + tid; q < M.b_rp[k + 1]; q += BLOCK) {
                const int32_t j = M.b_ci[q];
                const bool fresh = mark[j] != tag;
                if (fresh) { mark[j] = tag; ++mine; }
                if (NUM) acc[j] = sadd(fresh ? szero<T>() : acc[j], smul(a, b_v[q]));
            }
            __syncthreads();
        }
        if (!NUM) {
            if (mine) atomicAdd(&total, mine);
            __syncthreads();
            if (tid == 0) cnt[row] = total;
            __syncthreads();
            continue;
        }
        // the marked columns in ascending order: BLOCK columns per step, ranked by ballot within a wavefront
        int64_t at = c_rp[row];
        for (int64_t c0 = 0; c0 < ncB; c0 += BLOCK) {
            const int64_t j = c0 + tid;
            const bool f = j < ncB && mark[j] == tag;
            const unsigned long long b = __ballot(f);
            if (lane == 0) wtot[wave] = __popcll(b);
            __syncthreads();
            int before = __popcll(b & ((1ull << lane) - 1ull)), all = 0;
            for (int w = 0; w < BLOCK / SPG_WAVE; ++w) { if (w < wave) before += wtot[w]; all += wtot[w]; }
            if (f) { c_ci[at + before] = (int32_t)j; c_v[at + before] = acc[j]; }
            at += all;
            __syncthreads();
        }
    }
}

template <class T>
int spgemm_typed(sprs_ctx *c, const char *who, int64_t nrA, int64_t nrB, int64_t ncB, const int32_t *a_rp, const int32_t *a_ci, const T *a_v,
                 const int32_t *b_rp, const int32_t *b_ci, const T *b_v, int32_t **c_rp, int32_t **c_ci, T **c_v, int64_t *c_nnz, int64_t *info) {
    *c_rp = nullptr; *c_ci = nullptr; *c_v = nullptr; *c_nnz = 0;
    if (nrA > (int64_t)INT32_MAX || nrB > (int64_t)INT32_MAX || ncB > (int64_t)INT32_MAX) {
        snprintf(c->err, sizeof(c->err), "%s: more than 2^31 - 1 rows or columns", who);
        return SPRS_INVALID_ARGUMENT;
    }
    const Operands M{a_rp, a_ci, b_rp, b_ci};
    const int gA = (int)std::max<int64_t>((nrA + BLOCK - 1) / BLOCK, 1), gB = (int)std::max<int64_t>((nrB + BLOCK - 1) / BLOCK, 1);
    DevBufs tmp;
    uint8_t *path;
    int *bad;
    int32_t *pos[3], *list[3], *cnt, *rp;
    int64_t *rp64;
    SPRS_TRY(tmp.alloc(c, &path, (size_t)nrA + 1));          // (the scans read nrA + 1 elements: the last one is no path)
    SPRS_TRY(tmp.alloc(c, &bad, 4));
    for (int w = 0; w < 3; ++w) SPRS_TRY(tmp.alloc(c, &pos[w], (size_t)nrA + 1));
    SPRS_TRY(tmp.alloc(c, &cnt, (size_t)nrA + 1));
    SPRS_TRY(tmp.alloc(c, &rp64, (size_t)nrA + 1));
    SPRS_TRY(tmp.alloc(c, &rp, (size_t)nrA + 1));
    // bound, the check of B, the lists
    SPRS_HIP_TRY(c, hipMemsetAsync(bad, 0x7f, sizeof(int) * 4, c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(path, 0xff, (size_t)nrA + 1, c->stream));
    hipLaunchKernelGGL(spg_bound_kernel, dim3(gA), dim3(BLOCK), 0, c->stream, nrA, nrB, a_rp, a_ci, b_rp, (int64_t)SPG_SHORT_MAX, (int64_t)table_max<T>(), path, bad);
    hipLaunchKernelGGL(spg_check_b_kernel, dim3(gB), dim3(BLOCK), 0, c->stream, nrB, ncB, b_rp, b_ci, bad);
    SPRS_HIP_TRY(c, hipGetLastError());
    size_t scan_bytes = 0, s64_bytes = 0;
    {
        auto it = rocprim::make_transform_iterator(path, IsPath{0});
        SPRS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, it, pos[0], (int32_t)0, (size_t)nrA + 1, rocprim::plus<int32_t>(), c->stream));
        SPRS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, s64_bytes, cnt, rp64, (int64_t)0, (size_t)nrA + 1, rocprim::plus<int64_t>(), c->stream));
    }
    char *scratch;
    SPRS_TRY(tmp.alloc(c, &scratch, std::max(scan_bytes, s64_bytes)));
    for (int w = 0; w < 3; ++w) {
        auto it = rocprim::make_transform_iterator(path, IsPath{w});
        SPRS_HIP_TRY(c, rocprim::exclusive_scan(scratch, scan_bytes, it, pos[w], (int32_t)0, (size_t)nrA + 1, rocprim::plus<int32_t>(), c->stream));
    }
    int32_t n_list[3] = {0, 0, 0};
    int h_bad[4];
    for (int w = 0; w < 3; ++w) SPRS_HIP_TRY(c, hipMemcpyAsync(&n_list[w], pos[w] + nrA, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_bad[0] < (int)0x7f7f7f7f) {
        snprintf(c->err, sizeof(c->err), "%s: row %d of the left operand has a column index outside [0, %lld)", who, h_bad[0], (long long)nrB);
        return SPRS_INVALID_ARGUMENT;
    }
    if (h_bad[1] < (int)0x7f7f7f7f) {
        snprintf(c->err, sizeof(c->err), "%s: the column indices of row %d of the right operand are not strictly ascending inside [0, %lld)", who,
                 h_bad[1], (long long)ncB);
        return SPRS_INVALID_ARGUMENT;
    }
    if ((int64_t)n_list[0] + n_list[1] + n_list[2] != nrA) {
        snprintf(c->err, sizeof(c->err), "%s: internal error: the path lists hold %lld of %lld rows", who,
                 (long long)n_list[0] + n_list[1] + n_list[2], (long long)nrA);
        return SPRS_ERR_HIP;
    }
    for (int w = 0; w < 3; ++w) SPRS_TRY(tmp.alloc(c, &list[w], (size_t)n_list[w]));
    if (nrA) {
        hipLaunchKernelGGL(spg_fill_lists_kernel, dim3(gA), dim3(BLOCK), 0, c->stream, nrA, path, pos[0], pos[1], pos[2], list[0], list[1], list[2]);
        SPRS_HIP_TRY(c, hipGetLastError());
    }
    // the fallback's scratch: G workgroups of ncB marks (and, for the numeric pass, accumulators)
    int G = 0;
    uint32_t *mark = nullptr;
    T *acc = nullptr;
    if (n_list[2] > 0) {
        const size_t per = (size_t)std::max<int64_t>(ncB, 1) * (sizeof(T) + sizeof(uint32_t));
        G = (int)std::min<size_t>(std::max<size_t>(SPG_FB_BYTES / per, 1), (size_t)std::min<int>(SPG_FB_GROUPS, n_list[2]));
        SPRS_TRY(tmp.alloc(c, &mark, (size_t)G * (size_t)ncB));
        SPRS_TRY(tmp.alloc(c, &acc, (size_t)G * (size_t)ncB));
    }
    const int g_short = (n_list[0] + SPG_SHORT_ROWS - 1) / SPG_SHORT_ROWS;
    // symbolic
    SPRS_HIP_TRY(c, hipMemsetAsync(cnt, 0, sizeof(int32_t) * ((size_t)nrA + 1), c->stream));
    if (n_list[0])
        hipLaunchKernelGGL((spg_short_kernel<T, false>), dim3(g_short), dim3(SPG_WAVE), 0, c->stream, (int)n_list[0], list[0], M, a_v, b_v, cnt, nullptr, nullptr, (T *)nullptr, bad);
    if (n_list[1])
        hipLaunchKernelGGL((spg_table_kernel<T, false>), dim3(n_list[1]), dim3(BLOCK), 0, c->stream, list[1], M, a_v, b_v, cnt, nullptr, nullptr, (T *)nullptr, bad);
    if (n_list[2]) {
        SPRS_HIP_TRY(c, hipMemsetAsync(mark, 0, sizeof(uint32_t) * (size_t)G * (size_t)ncB, c->stream));
        hipLaunchKernelGGL((spg_fallback_kernel<T, false>), dim3(G), dim3(BLOCK), 0, c->stream, (int)n_list[2], list[2], M, a_v, b_v, ncB, mark, acc, cnt, nullptr, nullptr, (T *)nullptr);
    }
    SPRS_HIP_TRY(c, hipGetLastError());
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(scratch, s64_bytes, cnt, rp64, (int64_t)0, (size_t)nrA + 1, rocprim::plus<int64_t>(), c->stream));
    int64_t total = -1;
    SPRS_HIP_TRY(c, hipMemcpyAsync(&total, rp64 + nrA, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_bad[2] < (int)0x7f7f7f7f) {
        snprintf(c->err, sizeof(c->err), "%s: internal error: a table sized by the bound filled", who);
        return SPRS_ERR_HIP;
    }
    if (total < 0 || total > (int64_t)INT32_MAX) {
        snprintf(c->err, sizeof(c->err), "%s: the product has more than 2^31 - 1 stored entries", who);
        return SPRS_INVALID_ARGUMENT;
    }
    // numeric
    int32_t *ci;
    T *vv;
    SPRS_TRY(tmp.alloc(c, &ci, (size_t)total));
    SPRS_TRY(tmp.alloc(c, &vv, (size_t)total));
    hipLaunchKernelGGL(spg_narrow_kernel, dim3((int)(((int64_t)nrA + 1 + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, c->stream, nrA + 1, rp64, rp);
    if (n_list[0])
        hipLaunchKernelGGL((spg_short_kernel<T, true>), dim3(g_short), dim3(SPG_WAVE), 0, c->stream, (int)n_list[0], list[0], M, a_v, b_v, cnt, rp, ci, vv, bad);
    if (n_list[1])
        hipLaunchKernelGGL((spg_table_kernel<T, true>), dim3(n_list[1]), dim3(BLOCK), 0, c->stream, list[1], M, a_v, b_v, cnt, rp, ci, vv, bad);
    if (n_list[2]) {
        SPRS_HIP_TRY(c, hipMemsetAsync(mark, 0, sizeof(uint32_t) * (size_t)G * (size_t)ncB, c->stream));
        hipLaunchKernelGGL((spg_fallback_kernel<T, true>), dim3(G), dim3(BLOCK), 0, c->stream, (int)n_list[2], list[2], M, a_v, b_v, ncB, mark, acc, cnt, rp, ci, vv);
    }
    SPRS_HIP_TRY(c, hipGetLastError());
    SPRS_HIP_TRY(c, hipMemcpyAsync(h_bad, bad, sizeof(h_bad), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_bad[2] < (int)0x7f7f7f7f) {
        snprintf(c->err, sizeof(c->err), "%s: internal error: a table sized by the bound filled", who);
        return SPRS_ERR_HIP;
    }
    if (info) {
        info[0] = n_list[0]; info[1] = n_list[1]; info[2] = n_list[2];
        info[3] = SPG_SHORT_MAX; info[4] = table_max<T>();
    }
    tmp.release(rp); tmp.release(ci); tmp.release(vv);
    *c_rp = rp; *c_ci = ci; *c_v = vv; *c_nnz = total;
    return SPRS_OK;
}

template <class T, class CT>
int matmul_typed(const sprs_csr *A, const sprs_csr *B, int (*create_dev)(sprs_ctx *, int64_t, int64_t, int64_t, const int32_t *, const int32_t *, const CT *, int, sprs_csr **),
                 sprs_csr **out, int64_t *info) {
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    int32_t *rp, *ci;
    T *vv;
    int64_t nnz;
    SPRS_TRY(spgemm_dev<T>(c, "sprs_csr_matmul", A->nrows, B->nrows, B->ncols, A->row_ptr, A->col_idx, (const T *)A->val, B->row_ptr, B->col_idx,
                           (const T *)B->val, &rp, &ci, &vv, &nnz, info));
    DevBufs own;                                                       // released if creation fails
    own.p = {(void *)rp, (void *)ci, (void *)vv};
    sprs_csr *H = nullptr;
    SPRS_TRY(create_dev(c, A->nrows, B->ncols, nnz, rp, ci, reinterpret_cast<const CT *>(vv), 1, &H));
    H->owns_arrays = true;                                             // adopted, and from here on released with the handle
    own.p.clear();
    *out = H;
    return SPRS_OK;
}

}  // namespace

namespace sprs {

template <class T>
int spgemm_dev(sprs_ctx *c, const char *who, int64_t nrA, int64_t nrB, int64_t ncB, const int32_t *a_rp, const int32_t *a_ci, const T *a_v,
               const int32_t *b_rp, const int32_t *b_ci, const T *b_v, int32_t **c_rp, int32_t **c_ci, T **c_v, int64_t *c_nnz, int64_t *info) {
    return spgemm_typed<T>(c, who, nrA, nrB, ncB, a_rp, a_ci, a_v, b_rp, b_ci, b_v, c_rp, c_ci, c_v, c_nnz, info);
}
#define SPRS_SPGEMM_INST(T)                                                                                                                  \
    template int spgemm_dev<T>(sprs_ctx *, const char *, int64_t, int64_t, int64_t, const int32_t *, const int32_t *, const T *, const int32_t *, \
                               const int32_t *, const T *, int32_t **, int32_t **, T **, int64_t *, int64_t *);
SPRS_SPGEMM_INST(double)
SPRS_SPGEMM_INST(cplx)
SPRS_SPGEMM_INST(float)
SPRS_SPGEMM_INST(cplxf)

}  // namespace sprs

extern "C" {

int sprs_csr_matmul(const sprs_csr *A, const sprs_csr *B, sprs_csr **out, int64_t *info) {
    if (!A || !B || !out) return SPRS_INVALID_ARGUMENT;
    *out = nullptr;
    SPRS_TRY(single_gpu_only(A, "sprs_csr_matmul", B));
    if (A->ctx != B->ctx || A->dtype != B->dtype) {
        snprintf(A->ctx->err, sizeof(A->ctx->err), "sprs_csr_matmul: the operands must have the same scalar type and context");
        return SPRS_INVALID_ARGUMENT;
    }
    if (A->ncols != B->nrows) return SPRS_DIM_MISMATCH;
    try {
        switch (A->dtype) {
            case DT_D: return matmul_typed<double, double>(A, B, sprs_csr_create_dev_d, out, info);
            case DT_Z: return matmul_typed<cplx, sprs_c64>(A, B, sprs_csr_create_dev_z, out, info);
            case DT_S: return matmul_typed<float, float>(A, B, sprs_csr_create_dev_s, out, info);
            case DT_C: return matmul_typed<cplxf, sprs_c32>(A, B, sprs_csr_create_dev_c, out, info);
        }
    } catch (...) { return SPRS_ERR_HIP; }
    return SPRS_INVALID_ARGUMENT;
}

}  // extern "C"
