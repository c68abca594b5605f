// Orderings: a graph colouring of a square operator's pattern (sprs_csr_color) and the symmetric permutation
// B = P A P^T as an ordinary handle of its own (sprs_csr_permute).  The header states both as loops; ilu0.hip uses both for
// sprs_ilu0_create_ordered.  No reference analogue.
//
// Colouring.  The graph is the pattern of A + A^T without the diagonal; the second half is built here by count / scan / fill,
// its neighbour lists in whatever order the fill's slot counters hand out: a round reads a list as a set (a maximum test and
// an OR of colour bits), so the colours do not depend on that order.  The rule is greedy first-fit in decreasing (w(i), i);
// the device runs Jones-Plassmann rounds, one launch each: an uncoloured vertex that beats every uncoloured neighbour takes
// the smallest colour no coloured neighbour has.  The vertices of one round are independent, so the round runs in place.
// What keeps it deterministic whatever the launch geometry: a colour written in round r is stored as the negative code
// -(2 colour + 2 + (r & 1)), which readers of round r take for "uncoloured" (as it was when the round began) and readers of
// round r + 1 for the colour; the vertex's own lane replaces the code by the colour in round r + 1.  A vertex's two neighbour
// lists are walked twice (the maximum test, then the colour bits, a 64-colour window at a time): by its own lane when they hold
// at most 64 entries, by its whole wavefront with a strided loop when they hold more.
//
// Permutation.  The inverse permutation (one kernel), the permuted row lengths and their scan (rocprim), then one wavefront
// per row of B: gather the row of A, relabel the columns through the inverse, and place every entry at the rank of its new
// column: the entries with a smaller key, and those with an equal key stored before it.  That is the position of the STABLE sort,
// so a row of A may be stored in any order and a duplicate column keeps its stored order (as in the adjoint), every slot of B is
// written exactly once, and distinct columns give any correct sort's bits.  A row of up to 64 entries holds its keys in
// registers, one per lane, and ranks them by 64 shuffles; a longer row re-reads its keys from memory, 64 entries at a time
// (len^2 / 64 loads per lane: the set-up cost of a dense row, not of a sparse one).  Values are moved as bit patterns of
// their size, so the kernels do not depend on the scalar type.
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "device.hpp"

using namespace sprs;

namespace {

// ---- colouring
// the colour of a vertex as round `parity` sees it: -1 while it had none when the round began
__device__ __forceinline__ int jp_decode(int v, int parity) {
    if (v >= -1) return v;
    const int e = -v - 2;
    return (e & 1) == parity ? -1 : e >> 1;
}

__global__ __launch_bounds__(BLOCK) void tr_count_kernel(int n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, int32_t *__restrict__ cnt) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (i >= n) return;
    for (int k = rp[i]; k < rp[i + 1]; ++k) {
        const int c = ci[k];
        if ((unsigned)c < (unsigned)n && c != i) atomicAdd(cnt + c, 1);
    }
}

__global__ __launch_bounds__(BLOCK) void tr_fill_kernel(int n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                        const int32_t *__restrict__ tp, int32_t *__restrict__ cur, int32_t *__restrict__ tj) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (i >= n) return;
    for (int k = rp[i]; k < rp[i + 1]; ++k) {
        const int c = ci[k];
        if ((unsigned)c < (unsigned)n && c != i) tj[tp[c] + atomicAdd(cur + c, 1)] = i;
    }
}

// One vertex's two neighbour lists as one index range: entry k of [0, deg) is ci[a0 + k] or tj[t0 + (k - (a1 - a0))].
struct JpRow {
    int a0, a1, t0, t1;
    __device__ __forceinline__ int deg() const { return (a1 - a0) + (t1 - t0); }
    __device__ __forceinline__ int at(int k, const int32_t *__restrict__ ci, const int32_t *__restrict__ tj) const {
        return k < a1 - a0 ? ci[a0 + k] : tj[t0 + (k - (a1 - a0))];
    }
};

// neighbour j of vertex i (weight wi) is uncoloured in this round and stronger
__device__ __forceinline__ bool jp_beats(int j, int i, uint64_t wi, int n, uint64_t seed, int parity, const int32_t *color) {
    if ((unsigned)j >= (unsigned)n || j == i || jp_decode(color[j], parity) >= 0) return false;
    const uint64_t wj = vertex_key(seed, j);
    return wj > wi || (wj == wi && j > i);
}

// the bit of neighbour j's colour in the window [base, base + 64), 0 outside it
__device__ __forceinline__ uint64_t jp_bit(int j, int i, int n, int base, int parity, const int32_t *color) {
    if ((unsigned)j >= (unsigned)n || j == i) return 0;
    const int cj = jp_decode(color[j], parity) - base;
    return cj >= 0 && cj < 64 ? 1ull << cj : 0;
}

// One Jones-Plassmann round.  A vertex of at most 64 neighbour entries is walked by its own lane; the longer ones of a wavefront
// are then taken one after the other by the whole wavefront, the lanes striding the lists (the verdict by a ballot, the colour
// mask by an OR across the lanes).  stat[0] += the vertices coloured, stat[1] = max(stat[1], colour + 1).
__global__ __launch_bounds__(BLOCK) void jp_round_kernel(int n, uint64_t seed, int parity, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                         const int32_t *__restrict__ tp, const int32_t *__restrict__ tj, int32_t *color, unsigned int *stat) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x, lane = threadIdx.x & (WAVE - 1);
    int took = 0;                                                      // colour + 1 where this lane's vertex was coloured
    JpRow R{0, 0, 0, 0};
    bool open = false;                                                 // uncoloured when the round began
    if (i < n) {
        const int v = color[i];
        if (v < -1) {
            if (((-v - 2) & 1) != parity) color[i] = (-v - 2) >> 1;    // coloured in the round before: the code becomes the colour
        } else if (v == -1) {
            open = true;
            R = JpRow{rp[i], rp[i + 1], tp[i], tp[i + 1]};
        }
    }
    const int deg = R.deg();
    if (open && deg <= WAVE) {
        const uint64_t wi = vertex_key(seed, i);
        bool top = true;
        for (int k = 0; k < deg && top; ++k) top = !jp_beats(R.at(k, ci, tj), i, wi, n, seed, parity, color);
        if (top) {
            int col = -1;
            for (int base = 0; col < 0; base += 64) {
                uint64_t used = 0;
                for (int k = 0; k < deg; ++k) used |= jp_bit(R.at(k, ci, tj), i, n, base, parity, color);
                if (~used) col = base + __builtin_ctzll(~used);
            }
            color[i] = -(2 * col + 2 + parity);
            took = col + 1;
        }
    }
    for (uint64_t todo = __ballot(open && deg > WAVE); todo; todo &= todo - 1) {   // (wave-uniform)
        const int src = __builtin_ctzll(todo);
        const int r = __shfl(i, src);
        const JpRow Q{__shfl(R.a0, src), __shfl(R.a1, src), __shfl(R.t0, src), __shfl(R.t1, src)};
        const int qdeg = Q.deg();
        const uint64_t wr = vertex_key(seed, r);
        bool beaten = false;
        for (int k = lane; k < qdeg; k += WAVE) beaten |= jp_beats(Q.at(k, ci, tj), r, wr, n, seed, parity, color);
        if (__ballot(beaten)) continue;
        int col = -1;
        for (int base = 0; col < 0; base += 64) {
            uint64_t used = 0;
            for (int k = lane; k < qdeg; k += WAVE) used |= jp_bit(Q.at(k, ci, tj), r, n, base, parity, color);
            for (int d = WAVE / 2; d; d >>= 1) used |= (uint64_t)__shfl_xor((unsigned long long)used, d);
            if (~used) col = base + __builtin_ctzll(~used);
        }
        if (lane == src) {
            color[r] = -(2 * col + 2 + parity);
            took = col + 1;
        }
    }
    const int cnt = __popcll(__ballot(took != 0));
    if (!cnt) return;
    int mx = took;
    for (int d = WAVE / 2; d; d >>= 1) mx = max(mx, __shfl_xor(mx, d));
    if (lane == 0) {
        atomicAdd(stat, (unsigned)cnt);
        atomicMax(stat + 1, (unsigned)mx);
    }
}

// ---- permutation
__global__ __launch_bounds__(BLOCK) void perm_inverse_kernel(int n, const int32_t *__restrict__ perm, const int32_t *__restrict__ rp,
                                                             int32_t *__restrict__ inv, int32_t *__restrict__ len) {
    const int p = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (p == n) len[n] = 0;
    if (p >= n) return;
    const int i = perm[p];                                             // (perm_check: 0 <= i < n, no duplicates)
    inv[i] = p;
    len[p] = rp[i + 1] - rp[i];
}

struct Bits16 { uint64_t a, b; };

// row p of B by one wavefront, every entry at its stable rank; a column of A outside [0, n) (an adopted array changed after creation) keeps its value as key
template <class U>
__global__ __launch_bounds__(BLOCK) void permute_rows_kernel(int n, const int32_t *__restrict__ perm, const int32_t *__restrict__ inv,
                                                             const int32_t *__restrict__ a_rp, const int32_t *__restrict__ a_ci, const U *__restrict__ a_v,
                                                             const int32_t *__restrict__ b_rp, int32_t *__restrict__ b_ci, U *__restrict__ b_v,
                                                             int32_t *__restrict__ src) {
    const int p = (int)blockIdx.x * NWAVE + (int)(threadIdx.x >> 6), lane = threadIdx.x & (WAVE - 1);
    if (p >= n) return;
    const int i = perm[p], a0 = a_rp[i], len = a_rp[i + 1] - a0, b0 = b_rp[p];
    auto key_of = [&](int e) { const int c = a_ci[a0 + e]; return (unsigned)c < (unsigned)n ? inv[c] : c; };
    if (len <= WAVE) {
        const int key = lane < len ? key_of(lane) : INT32_MAX;
        int rank = 0;
        for (int t = 0; t < len; ++t) { const int kt = __shfl(key, t); rank += kt < key || (kt == key && t < lane); }
        if (lane < len) {
            b_ci[b0 + rank] = key; b_v[b0 + rank] = a_v[a0 + lane];
            if (src) src[b0 + rank] = a0 + lane;
        }
        return;
    }
    for (int e = lane; e < len; e += WAVE) {
        const int key = key_of(e);
        int rank = 0;
        for (int t = 0; t < len; ++t) { const int kt = key_of(t); rank += kt < key || (kt == key && t < e); }
        b_ci[b0 + rank] = key; b_v[b0 + rank] = a_v[a0 + e];
        if (src) src[b0 + rank] = a0 + e;
    }
}

int square_single(const sprs_csr *A, const char *who) {
    SPRS_TRY(single_gpu_only(A, who));   // (before the shape: a row block with a halo has more columns than rows)
    return A->nrows == A->ncols ? SPRS_OK : SPRS_NOT_SQUARE;
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)std::max<int64_t>((n + per - 1) / per, 1); }

}  // namespace

namespace sprs {

int perm_check(const sprs_ctx *c, const char *who, const int32_t *perm, size_t len, int64_t n) {
    if (len != (size_t)n) return refuse(c, who, "the permutation has %zu entries, the matrix %lld rows", len, (long long)n);
    std::vector<bool> seen((size_t)n, false);
    for (size_t p = 0; p < len; ++p) {
        const int64_t i = perm[p];
        if (i < 0 || i >= n) return refuse(c, who, "perm[%zu] = %lld is outside [0, %lld)", p, (long long)i, (long long)n);
        if (seen[(size_t)i]) return refuse(c, who, "perm[%zu] = %lld appears twice: not a permutation", p, (long long)i);
        seen[(size_t)i] = true;
    }
    return SPRS_OK;
}

std::vector<int32_t> color_major_perm(const std::vector<int32_t> &colors, int64_t ncolors) {
    std::vector<int32_t> ptr, perm;
    group_by_level(colors, (int32_t)ncolors, ptr, perm);
    return perm;
}

int csr_color_host(const sprs_csr *A, uint64_t seed, std::vector<int32_t> &colors, int64_t *ncolors, int64_t *rounds) {
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    const int64_t n = A->nrows;
    colors.assign((size_t)n, -1);
    if (ncolors) *ncolors = 0;
    if (rounds) *rounds = 0;
    if (!n) return SPRS_OK;
    DevBufs tmp;
    int32_t *cnt, *tp, *tj, *color;
    unsigned int *stat;
    char *scratch;
    SPRS_TRY(tmp.alloc(c, &cnt, (size_t)n + 1));
    SPRS_TRY(tmp.alloc(c, &tp, (size_t)n + 1));
    SPRS_TRY(tmp.alloc(c, &tj, (size_t)A->nnz));
    SPRS_TRY(tmp.alloc(c, &color, (size_t)n));
    SPRS_TRY(tmp.alloc(c, &stat, 2));
    const dim3 grid(blocks_of(n, BLOCK)), block(BLOCK);
    // the other half of the graph: the pattern of A^T without the diagonal
    SPRS_HIP_TRY(c, hipMemsetAsync(cnt, 0, sizeof(int32_t) * ((size_t)n + 1), c->stream));
    hipLaunchKernelGGL(tr_count_kernel, grid, block, 0, c->stream, (int)n, A->row_ptr, A->col_idx, cnt);
    size_t scan_bytes = 0;
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, cnt, tp, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), c->stream));
    SPRS_TRY(tmp.alloc(c, &scratch, scan_bytes));
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(scratch, scan_bytes, cnt, tp, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(cnt, 0, sizeof(int32_t) * ((size_t)n + 1), c->stream));
    hipLaunchKernelGGL(tr_fill_kernel, grid, block, 0, c->stream, (int)n, A->row_ptr, A->col_idx, tp, cnt, tj);
    SPRS_HIP_TRY(c, hipGetLastError());
    // the rounds: the host reads the two counter words after each
    SPRS_HIP_TRY(c, hipMemsetAsync(color, 0xFF, sizeof(int32_t) * (size_t)n, c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(stat, 0, sizeof(unsigned int) * 2, c->stream));
    unsigned int h_stat[2] = {0, 0};
    int64_t r = 0;
    while ((int64_t)h_stat[0] < n) {
        if (r >= n) {                    // (cannot happen: the largest uncoloured vertex is coloured in every round)
            snprintf(c->err, sizeof(c->err), "sprs_csr_color: %lld rounds coloured %u of %lld vertices", (long long)r, h_stat[0], (long long)n);
            return SPRS_ERR_HIP;
        }
        hipLaunchKernelGGL(jp_round_kernel, grid, block, 0, c->stream, (int)n, seed, (int)(r & 1), A->row_ptr, A->col_idx, tp, tj, color, stat);
        SPRS_HIP_TRY(c, hipGetLastError());
        SPRS_HIP_TRY(c, hipMemcpyAsync(h_stat, stat, sizeof(h_stat), hipMemcpyDeviceToHost, c->stream));
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        ++r;
    }
    SPRS_HIP_TRY(c, hipMemcpyAsync(colors.data(), color, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int32_t &v : colors) if (v < -1) v = (-v - 2) >> 1;           // the last round's codes
    if (ncolors) *ncolors = h_stat[1];
    if (rounds) *rounds = r;
    return SPRS_OK;
}

int csr_permute_arrays(const sprs_csr *A, const int32_t *perm_dev, int32_t **rp_out, int32_t **ci_out, void **val_out, int32_t **src_out) {
    sprs_ctx *c = A->ctx;
    const int64_t n = A->nrows, nnz = A->nnz;
    const size_t es = dtype_size(A->dtype);
    DevBufs tmp;
    int32_t *inv, *len, *rp, *ci, *src = nullptr;
    char *val, *scratch;
    SPRS_TRY(tmp.alloc(c, &inv, (size_t)n));
    SPRS_TRY(tmp.alloc(c, &len, (size_t)n + 1));
    SPRS_TRY(tmp.alloc(c, &rp, (size_t)n + 1));
    SPRS_TRY(tmp.alloc(c, &ci, (size_t)nnz));
    SPRS_TRY(tmp.alloc(c, &val, es * (size_t)nnz));
    if (src_out) SPRS_TRY(tmp.alloc(c, &src, (size_t)nnz));
    hipLaunchKernelGGL(perm_inverse_kernel, dim3(blocks_of(n + 1, BLOCK)), dim3(BLOCK), 0, c->stream, (int)n, perm_dev, A->row_ptr, inv, len);
    SPRS_HIP_TRY(c, hipGetLastError());
    size_t scan_bytes = 0;
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, scan_bytes, len, rp, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), c->stream));
    SPRS_TRY(tmp.alloc(c, &scratch, scan_bytes));
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(scratch, scan_bytes, len, rp, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), c->stream));
    if (n) {
        const dim3 grid(blocks_of(n, NWAVE)), block(BLOCK);
        if (es == 4)
            hipLaunchKernelGGL((permute_rows_kernel<uint32_t>), grid, block, 0, c->stream, (int)n, perm_dev, inv, A->row_ptr, A->col_idx, (const uint32_t *)A->val, rp, ci, (uint32_t *)val, src);
        else if (es == 8)
            hipLaunchKernelGGL((permute_rows_kernel<uint64_t>), grid, block, 0, c->stream, (int)n, perm_dev, inv, A->row_ptr, A->col_idx, (const uint64_t *)A->val, rp, ci, (uint64_t *)val, src);
        else
            hipLaunchKernelGGL((permute_rows_kernel<Bits16>), grid, block, 0, c->stream, (int)n, perm_dev, inv, A->row_ptr, A->col_idx, (const Bits16 *)A->val, rp, ci, (Bits16 *)val, src);
        SPRS_HIP_TRY(c, hipGetLastError());
    }
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    tmp.release(rp); tmp.release(ci); tmp.release(val);
    *rp_out = rp; *ci_out = ci; *val_out = val;
    if (src_out) { tmp.release(src); *src_out = src; }
    return SPRS_OK;
}

}  // namespace sprs

extern "C" {

int sprs_csr_color(const sprs_csr *A, uint64_t seed, int32_t *colors_host, int64_t *ncolors_out, int64_t *rounds_out) {
    if (!A || (!colors_host && A->nrows)) return SPRS_INVALID_ARGUMENT;
    SPRS_TRY(square_single(A, "sprs_csr_color"));
    try {
        std::vector<int32_t> colors;
        SPRS_TRY(csr_color_host(A, seed, colors, ncolors_out, rounds_out));
        std::copy(colors.begin(), colors.end(), colors_host);
        return SPRS_OK;
    } catch (...) { return SPRS_ERR_HIP; }
}

int sprs_csr_permute(const sprs_csr *A, const int32_t *perm_host, size_t perm_len, sprs_csr **out) {
    if (!A || !out || (!perm_host && perm_len)) return SPRS_INVALID_ARGUMENT;
    *out = nullptr;
    SPRS_TRY(square_single(A, "sprs_csr_permute"));
    try {
        sprs_ctx *c = A->ctx;
        SPRS_TRY(perm_check(c, "sprs_csr_permute", perm_host, perm_len, A->nrows));
        CtxLock lock(c);
        SPRS_HIP_TRY(c, hipSetDevice(c->device));
        DevBufs tmp;
        int32_t *perm, *rp = nullptr, *ci = nullptr;
        void *val = nullptr;
        SPRS_TRY(tmp.alloc(c, &perm, perm_len));
        if (perm_len) SPRS_HIP_TRY(c, hipMemcpyAsync(perm, perm_host, sizeof(int32_t) * perm_len, hipMemcpyHostToDevice, c->stream));
        SPRS_TRY(csr_permute_arrays(A, perm, &rp, &ci, &val, nullptr));
        tmp.p.push_back(rp); tmp.p.push_back(ci); tmp.p.push_back(val);   // released below once the handle owns them
        tmp.free(perm);
        const int64_t n = A->nrows, nnz = A->nnz;
        sprs_csr *H = nullptr;
        switch (A->dtype) {
            case DT_D: SPRS_TRY(sprs_csr_create_dev_d(c, n, n, nnz, rp, ci, (const double *)val, 1, &H)); break;
            case DT_Z: SPRS_TRY(sprs_csr_create_dev_z(c, n, n, nnz, rp, ci, (const sprs_c64 *)val, 1, &H)); break;
            case DT_S: SPRS_TRY(sprs_csr_create_dev_s(c, n, n, nnz, rp, ci, (const float *)val, 1, &H)); break;
            case DT_C: SPRS_TRY(sprs_csr_create_dev_c(c, n, n, nnz, rp, ci, (const sprs_c32 *)val, 1, &H)); break;
            default: return SPRS_INVALID_ARGUMENT;
        }
        H->owns_arrays = true;                                             // adopted, and from here on released with the handle
        tmp.release(rp); tmp.release(ci); tmp.release(val);
        *out = H;
        return SPRS_OK;
    } catch (...) { return SPRS_ERR_HIP; }
}

}  // extern "C"
