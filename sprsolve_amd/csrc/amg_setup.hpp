// The AMG hierarchy built in HBM (sprs_amg_create_dev): part of amg.hip, which includes this file once sprs_amg and
// its helpers are defined.  The header states the aggregation rule as loops; tests/_amg_par_ref.py restates it.
//
// One level, every array in HBM:
//   diag      the diagonal with its checks, |d_i| and q_i = (sum_j |a_ij|, left to right) / |d_i|, one lane per row; rho is a
//             rocprim::reduce of q under a NaN-keeping maximum, omega = 4 / (3 rho) on the host from that one scalar
//   graph     G as ONE neighbour list per vertex, (index, weight) pairs: the strong entries of row i in stored order, then the
//             strong entries of column i in whatever order the fill's slot counters hand out (count / scan / fill; the integer
//             atomics only count and hand out slots).  A pair of vertices coupled both ways appears twice in each list; every
//             reader takes a maximum over the list — of keys, or of (w, -j) — so neither the order nor the repeat reaches a result.
//   rounds    pass 1.  Three launches a round, so that no kernel reads what it writes: SETTLE (an undecided vertex that is
//             aggregated or has an aggregated neighbour stops being undecided; the undecided are counted), then the host reads
//             the counter; MAX (m1[k] = the undecided vertex of largest key in k's closed neighbourhood, for EVERY k: a path of
//             two edges may pass through a decided vertex); WIN (an undecided i whose closed neighbourhood holds no m1 above
//             its own key is the largest undecided vertex within distance 2: it becomes a root and takes its neighbours).  Two
//             winners of a round are more than two edges apart, so the sets they write are disjoint.
//   pass 2    against pass 1's array, into a second one; a free vertex without an aggregated neighbour is reported, not assumed away
//   numbering root flags, rocprim::exclusive_scan, agg[i] = id[root[i]]
//   the rest  T, A T (spgemm_dev), the prolongator formula in place, R = P^H (adjoint_dev), A P, R (A P), and the sliced-row
//             layout of A_l, P_l, R_l by slice widths / scan / fill with position = row
// Every walk over a neighbour list is nb_fold / nb_each: a list of at most 64 slots by the vertex's own lane, a longer one by the
// whole wavefront, so a hub does not serialise a round in one lane.
#pragma once
#include <rocprim/device/device_reduce.hpp>
#include <rocprim/device/device_scan.hpp>

namespace {

enum : int { SG_DIAG = 0, SG_GRAPH, SG_ROUNDS, SG_PASS2, SG_AT, SG_PROLONG, SG_ADJOINT, SG_AP, SG_RAP, SG_PACK, SG_LU };
static_assert(SG_LU + 1 == AMG_STAGES, "sprs_amg_setup_stage_ms documents this list");

// the vertex of larger (key, index); -1 stands for "none" and loses to every vertex
struct KeyMax {
    uint64_t seed;
    __device__ __forceinline__ int operator()(int a, int b) const {
        if (a < 0) return b;
        if (b < 0 || a == b) return a;
        const uint64_t wa = vertex_key(seed, a), wb = vertex_key(seed, b);
        return wa > wb || (wa == wb && a > b) ? a : b;
    }
};

// |a| with the host's bits: fabs, or the correctly rounded square root of re re + im im (f32: through f64, whose rounding to f32
// is the correctly rounded f32 root)
__device__ __forceinline__ double amg_mod(double a) { return fabs(a); }
__device__ __forceinline__ float amg_mod(float a) { return fabsf(a); }
__device__ __forceinline__ double amg_mod(cplx a) { return sqrt(ssq(a)); }
__device__ __forceinline__ float amg_mod(cplxf a) { return (float)sqrt((double)ssq(a)); }

template <class A>
__device__ __forceinline__ A shfl_xor_any(A v, int d) {
    static_assert(sizeof(A) % 4 == 0, "whole words");
    int w[sizeof(A) / 4];
    __builtin_memcpy(w, &v, sizeof(A));
#pragma unroll
    for (size_t t = 0; t < sizeof(A) / 4; ++t) w[t] = __shfl_xor(w[t], d);
    __builtin_memcpy(&v, w, sizeof(A));
    return v;
}
__device__ __forceinline__ int64_t shfl_i64(int64_t v, int src) {
    const int lo = __shfl((int)(uint32_t)(uint64_t)v, src), hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

// comb-fold of f(slot) over the list slots [g0, g1) of every active lane.  comb is associative and commutative (the lists are
// read as sets) and `neutral` is its neutral element, the same in every lane: on a long list each of the 64 lanes starts its
// partial from it, so nothing of a helping lane's own vertex enters the owner's result (what the owner adds for itself, it
// combines with the returned value).  EVERY lane of the wavefront calls this: the long lists are walked by all 64.
template <class ACC, class F, class COMB>
__device__ __forceinline__ ACC nb_fold(bool active, int64_t g0, int64_t g1, ACC neutral, F f, COMB comb) {
    const int lane = (int)threadIdx.x & (WAVE - 1);
    const bool wide = active && g1 - g0 > WAVE;
    ACC acc = neutral;
    if (active && !wide)
        for (int64_t k = g0; k < g1; ++k) acc = comb(acc, f(k));
    for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1) {     // (wave-uniform)
        const int src = __builtin_ctzll(todo);
        const int64_t q0 = shfl_i64(g0, src), q1 = shfl_i64(g1, src);
        ACC part = neutral;
        for (int64_t k = q0 + lane; k < q1; k += WAVE) part = comb(part, f(k));
        for (int d = WAVE / 2; d; d >>= 1) part = comb(part, shfl_xor_any(part, d));
        if (lane == src) acc = part;
    }
    return acc;
}

// f(slot, tag) for every slot of every active lane's list, tag being that lane's; the same split as nb_fold
template <class F>
__device__ __forceinline__ void nb_each(bool active, int64_t g0, int64_t g1, int tag, F f) {
    const int lane = (int)threadIdx.x & (WAVE - 1);
    const bool wide = active && g1 - g0 > WAVE;
    if (active && !wide)
        for (int64_t k = g0; k < g1; ++k) f(k, tag);
    for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1) {
        const int src = __builtin_ctzll(todo);
        const int64_t q0 = shfl_i64(g0, src), q1 = shfl_i64(g1, src);
        const int t = __shfl(tag, src);
        for (int64_t k = q0 + lane; k < q1; k += WAVE) f(k, t);
    }
}

// ---- the diagonal, |d|, the row quotients of omega
struct NanMax {      // a NaN wins and stays: any NaN quotient makes rho NaN, as the host loop does (that it is a NaN is reproduced; which
                     // NaN, sign and payload, depends on the reduction's order and is not)
    template <class R> __host__ __device__ R operator()(const R &a, const R &b) const { return a != a ? a : (b != b ? b : (a > b ? a : b)); }
};

template <class T>
__global__ __launch_bounds__(BLOCK) void su_diag_kernel(int n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ v,
                                                        T *__restrict__ diag, Real<T> *__restrict__ md, Real<T> *__restrict__ q, int *__restrict__ bad) {
    using R = Real<T>;
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (i >= n) return;
    const int p0 = rp[i], p1 = rp[i + 1];
    int lo = p0, hi = p1;                                    // the columns ascend strictly: lower_bound, as diag_pos
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ci[mid] < i) lo = mid + 1; else hi = mid;
    }
    T d = szero<T>();
    bool ok = lo < p1 && ci[lo] == i;
    if (ok) { d = v[lo]; ok = !bad_pivot(d); }
    diag[i] = d;
    if (!ok) { atomicMin(bad, i); md[i] = R(0); q[i] = R(0); return; }
    R s = R(0);
    for (int p = p0; p < p1; ++p) s = s + amg_mod(v[p]);
    const R m = amg_mod(d);
    md[i] = m;
    q[i] = s / m;
}

// ---- G
template <class T>
__device__ __forceinline__ bool su_strong(int i, int j, Real<T> sq, Real<T> th2, Real<T> mi, const Real<T> *md) { return j != i && sq >= th2 * (mi * md[j]); }

template <class T>
__global__ __launch_bounds__(BLOCK) void su_graph_count_kernel(int n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ v,
                                                               const Real<T> *__restrict__ md, Real<T> th2, int32_t *__restrict__ fwd, int32_t *cnt) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (i >= n) return;
    const Real<T> mi = md[i];
    int f = 0;
    for (int p = rp[i]; p < rp[i + 1]; ++p) {
        const int j = ci[p];
        if ((unsigned)j < (unsigned)n && su_strong<T>(i, j, ssq(v[p]), th2, mi, md)) { ++f; atomicAdd(cnt + j, 1); }
    }
    fwd[i] = f;
    if (f) atomicAdd(cnt + i, f);
}

template <class T>
__global__ __launch_bounds__(BLOCK) void su_graph_fill_kernel(int n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ v,
                                                              const Real<T> *__restrict__ md, Real<T> th2, const int32_t *__restrict__ fwd,
                                                              const int64_t *__restrict__ gp, int32_t *cur, int32_t *__restrict__ gj, Real<T> *__restrict__ gw) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (i >= n) return;
    const Real<T> mi = md[i];
    int64_t at = gp[i];
    for (int p = rp[i]; p < rp[i + 1]; ++p) {
        const int j = ci[p];
        const Real<T> sq = ssq(v[p]);
        if (!((unsigned)j < (unsigned)n && su_strong<T>(i, j, sq, th2, mi, md))) continue;
        gj[at] = j; gw[at] = sq; ++at;
        const int64_t d = gp[j] + fwd[j] + atomicAdd(cur + j, 1);
        gj[d] = i; gw[d] = sq;
    }
}

// ---- pass 1: one round = settle, (the host reads stat), max, win.  stat[0]: the undecided after settle, stat[1]: the winners
__global__ __launch_bounds__(BLOCK) void su_settle_kernel(int n, const int64_t *__restrict__ gp, const int32_t *__restrict__ gj, const int32_t *__restrict__ root,
                                                          uint8_t *undec, unsigned int *stat) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    bool open = i < n && undec[i] != 0;
    const bool own = open && root[i] >= 0;
    const int64_t g0 = open ? gp[i] : 0, g1 = open ? gp[i + 1] : 0;
    const int hit = nb_fold<int>(open && !own, g0, g1, 0, [&](int64_t k) { return root[gj[k]] >= 0 ? 1 : 0; }, [](int a, int b) { return a | b; });
    if (open && (own || hit)) { undec[i] = 0; open = false; }
    const int cnt = __popcll(__ballot(open));
    if (cnt && ((int)threadIdx.x & (WAVE - 1)) == 0) atomicAdd(stat, (unsigned)cnt);
}

__global__ __launch_bounds__(BLOCK) void su_max_kernel(int n, uint64_t seed, const int64_t *__restrict__ gp, const int32_t *__restrict__ gj,
                                                       const uint8_t *__restrict__ undec, int32_t *__restrict__ m1) {
    const int k = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    const bool in = k < n;
    const int64_t g0 = in ? gp[k] : 0, g1 = in ? gp[k + 1] : 0;
    const int self = in && undec[k] ? k : -1;
    const KeyMax larger{seed};
    const int m = larger(self, nb_fold<int>(in, g0, g1, -1, [&](int64_t s) { const int j = gj[s]; return undec[j] ? j : -1; }, larger));
    if (in) m1[k] = m;
}

__global__ __launch_bounds__(BLOCK) void su_win_kernel(int n, uint64_t seed, const int64_t *__restrict__ gp, const int32_t *__restrict__ gj,
                                                       const uint8_t *__restrict__ undec, const int32_t *__restrict__ m1, int32_t *root, unsigned int *stat) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    const bool open = i < n && undec[i] != 0;
    const int64_t g0 = open ? gp[i] : 0, g1 = open ? gp[i + 1] : 0;
    const KeyMax larger{seed};
    const int m = larger(open ? m1[i] : -1, nb_fold<int>(open, g0, g1, -1, [&](int64_t s) { return m1[gj[s]]; }, larger));
    const bool win = open && m == i;
    if (win) root[i] = i;
    nb_each(win, g0, g1, i, [&](int64_t s, int r) { root[gj[s]] = r; });   // (free until now: an undecided vertex has no aggregated neighbour)
    const int cnt = __popcll(__ballot(win));
    if (cnt && ((int)threadIdx.x & (WAVE - 1)) == 0) atomicAdd(stat + 1, (unsigned)cnt);
}

// ---- pass 2 against the snapshot `root`, into `out`
template <class R>
struct Best { R w; int j; };
template <class R>
struct BestMax {     // the largest w, ties to the smallest index; j < 0: none
    __device__ __forceinline__ Best<R> operator()(Best<R> a, Best<R> b) const {
        if (a.j < 0) return b;
        if (b.j < 0) return a;
        return a.w > b.w || (a.w == b.w && a.j < b.j) ? a : b;
    }
};

template <class R>
__global__ __launch_bounds__(BLOCK) void su_pass2_kernel(int n, const int64_t *__restrict__ gp, const int32_t *__restrict__ gj, const R *__restrict__ gw,
                                                         const int32_t *__restrict__ root, int32_t *__restrict__ out, int *__restrict__ bad) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    const int mine = i < n ? root[i] : 0;
    const bool free_v = i < n && mine < 0;
    const int64_t g0 = free_v ? gp[i] : 0, g1 = free_v ? gp[i + 1] : 0;
    const Best<R> none{R(-1), -1};
    const Best<R> b = nb_fold<Best<R>>(free_v, g0, g1, none, [&](int64_t s) { const int j = gj[s]; return root[j] >= 0 ? Best<R>{gw[s], j} : none; }, BestMax<R>{});
    if (i >= n) return;
    if (!free_v) { out[i] = mine; return; }
    if (b.j < 0) { atomicMin(bad, i); out[i] = -1; return; }
    out[i] = root[b.j];
}

// ---- numbering, T, the prolongator
__global__ __launch_bounds__(BLOCK) void su_rootflag_kernel(int n, const int32_t *__restrict__ root, int32_t *__restrict__ flag) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (i <= n) flag[i] = i < n && root[i] == i ? 1 : 0;
}

// agg[i] = id[root[i]]; T = (tip, agg, ones)
template <class T>
__global__ __launch_bounds__(BLOCK) void su_number_kernel(int n, const int32_t *__restrict__ root, const int32_t *__restrict__ id, int32_t *__restrict__ agg,
                                                          int32_t *__restrict__ tip, T *__restrict__ tv) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (i > n) return;
    tip[i] = i;
    if (i < n) { agg[i] = id[root[i]]; tv[i] = sone<T>(); }
}

// p_ic = t_ic - (omega (A T)_ic) / d_i on the pattern of A T, in place
template <class T>
__global__ __launch_bounds__(BLOCK) void su_prolong_kernel(int n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, T *__restrict__ v,
                                                           const int32_t *__restrict__ agg, const T *__restrict__ diag, Real<T> omega) {
    const int i = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (i >= n) return;
    const int a = agg[i];
    const T d = diag[i];
    for (int p = rp[i]; p < rp[i + 1]; ++p) {
        const T t = ci[p] == a ? sone<T>() : szero<T>();
        v[p] = ssub(t, sdiv(smulr(v[p], omega), d));
    }
}

// ---- the sliced-row layout, position = row
__global__ __launch_bounds__(BLOCK) void su_sell_width_kernel(int n, int npos, const int32_t *__restrict__ rp, int32_t *__restrict__ len, int64_t *__restrict__ slots) {
    const int p = (int)blockIdx.x * BLOCK + (int)threadIdx.x;          // (npos is a multiple of 64: a wavefront is one slice)
    if (p >= npos) return;
    const int l = p < n ? rp[p + 1] - rp[p] : 0;
    len[p] = l;
    int w = l;
    for (int d = WAVE / 2; d; d >>= 1) w = max(w, __shfl_xor(w, d));
    if ((p & (SELL_SLICE - 1)) == 0) slots[p >> 6] = (int64_t)w * SELL_SLICE;
}

template <class T>
__global__ __launch_bounds__(BLOCK) void su_sell_fill_kernel(int n, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci, const T *__restrict__ v,
                                                             const int64_t *__restrict__ sbase, int32_t *__restrict__ col, T *__restrict__ val) {
    const int p = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (p >= n) return;
    const int p0 = rp[p], l = rp[p + 1] - p0;
    const int64_t b = sbase[p >> 6] + (p & (SELL_SLICE - 1));
    for (int e = 0; e < l; ++e) { col[b + (int64_t)e * SELL_SLICE] = ci[p0 + e]; val[b + (int64_t)e * SELL_SLICE] = v[p0 + e]; }
}

inline dim3 su_grid(int64_t n) { return dim3((unsigned)std::max<int64_t>((n + BLOCK - 1) / BLOCK, 1)); }

// M = the packed layout of the CSR arrays (n rows); the padding slots hold column 0 and the value zero, as sell_pack's
template <class T>
int su_pack(sprs_ctx *c, SellMat &M, int32_t n, const int32_t *rp, const int32_t *ci, const T *v) {
    const int32_t nslice = (n + SELL_SLICE - 1) / SELL_SLICE;
    const int npos = nslice * SELL_SLICE;
    M.n = n; M.nslice = nslice;
    SPRS_HIP_TRY(c, hipMalloc((void **)&M.len, sizeof(int32_t) * ((size_t)npos + 2)));
    SPRS_HIP_TRY(c, hipMalloc((void **)&M.sbase, sizeof(int64_t) * ((size_t)nslice + 2)));
    DevBufs tmp;
    int64_t *slots;
    char *scratch;
    SPRS_TRY(tmp.alloc(c, &slots, (size_t)nslice + 1));
    SPRS_HIP_TRY(c, hipMemsetAsync(slots, 0, sizeof(int64_t) * ((size_t)nslice + 1), c->stream));
    if (npos) hipLaunchKernelGGL(su_sell_width_kernel, su_grid(npos), dim3(BLOCK), 0, c->stream, (int)n, npos, rp, M.len, slots);
    SPRS_HIP_TRY(c, hipGetLastError());
    size_t bytes = 0;
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, bytes, slots, M.sbase, (int64_t)0, (size_t)nslice + 1, rocprim::plus<int64_t>(), c->stream));
    SPRS_TRY(tmp.alloc(c, &scratch, bytes));
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(scratch, bytes, slots, M.sbase, (int64_t)0, (size_t)nslice + 1, rocprim::plus<int64_t>(), c->stream));
    int64_t total = 0;
    SPRS_HIP_TRY(c, hipMemcpyAsync(&total, M.sbase + nslice, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    SPRS_HIP_TRY(c, hipMalloc((void **)&M.col, sizeof(int32_t) * ((size_t)total + 2)));
    SPRS_HIP_TRY(c, hipMalloc(&M.val, sizeof(T) * ((size_t)total + 2)));
    SPRS_HIP_TRY(c, hipMemsetAsync(M.col, 0, sizeof(int32_t) * ((size_t)total + 2), c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(M.val, 0, sizeof(T) * ((size_t)total + 2), c->stream));
    if (n) hipLaunchKernelGGL((su_sell_fill_kernel<T>), su_grid(n), dim3(BLOCK), 0, c->stream, (int)n, rp, ci, v, (const int64_t *)M.sbase, M.col, (T *)M.val);
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

// The aggregates of one level: *agg_out (n entries, the caller's), the number of aggregates and pass 1's rounds.  md: |d_i|.
template <class T>
int su_aggregate(sprs_ctx *c, const DCsr<T> &A, const Real<T> *md, Real<T> theta, uint64_t seed, int32_t *agg, int32_t *tip, T *tv, int32_t *nc_out,
                 int64_t *rounds_out, SetupClock &clk) {
    using R = Real<T>;
    const int n = A.n;
    const R th2 = theta * theta;
    const dim3 grid = su_grid(n), grid1 = su_grid((int64_t)n + 1), block(BLOCK);
    DevBufs tmp;
    int32_t *fwd, *cnt, *gj, *root, *root2, *m1;
    int64_t *gp;
    R *gw;
    uint8_t *undec;
    unsigned int *stat;
    int *bad;
    char *scratch;
    SPRS_TRY(tmp.alloc(c, &fwd, (size_t)n));
    SPRS_TRY(tmp.alloc(c, &cnt, (size_t)n + 1));
    SPRS_TRY(tmp.alloc(c, &gp, (size_t)n + 1));
    SPRS_TRY(tmp.alloc(c, &gj, 2 * (size_t)A.nnz));          // every strong entry appears in two lists
    SPRS_TRY(tmp.alloc(c, &gw, 2 * (size_t)A.nnz));
    SPRS_TRY(tmp.alloc(c, &root, (size_t)n));
    SPRS_TRY(tmp.alloc(c, &root2, (size_t)n));
    SPRS_TRY(tmp.alloc(c, &m1, (size_t)n + 1));
    SPRS_TRY(tmp.alloc(c, &undec, (size_t)n));
    SPRS_TRY(tmp.alloc(c, &stat, 2));
    SPRS_TRY(tmp.alloc(c, &bad, 1));
    // G
    SPRS_HIP_TRY(c, hipMemsetAsync(cnt, 0, sizeof(int32_t) * ((size_t)n + 1), c->stream));
    hipLaunchKernelGGL((su_graph_count_kernel<T>), grid, block, 0, c->stream, n, A.ip, A.ix, A.v, md, th2, fwd, cnt);
    size_t b64 = 0, b32 = 0;
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, b64, cnt, gp, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), c->stream));
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(nullptr, b32, cnt, m1, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), c->stream));
    SPRS_TRY(tmp.alloc(c, &scratch, std::max(b64, b32)));
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(scratch, b64, cnt, gp, (int64_t)0, (size_t)n + 1, rocprim::plus<int64_t>(), c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(cnt, 0, sizeof(int32_t) * ((size_t)n + 1), c->stream));
    hipLaunchKernelGGL((su_graph_fill_kernel<T>), grid, block, 0, c->stream, n, A.ip, A.ix, A.v, md, th2, fwd, (const int64_t *)gp, cnt, gj, gw);
    SPRS_HIP_TRY(c, hipGetLastError());
    SPRS_TRY(clk.lap(c, SG_GRAPH));
    // pass 1
    SPRS_HIP_TRY(c, hipMemsetAsync(root, 0xFF, sizeof(int32_t) * (size_t)n, c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(undec, 1, (size_t)n, c->stream));
    SPRS_HIP_TRY(c, hipMemsetAsync(stat, 0, sizeof(unsigned int) * 2, c->stream));
    unsigned int h_stat[2] = {0, 0};
    int64_t rounds = 0;
    while (true) {
        hipLaunchKernelGGL(su_settle_kernel, grid, block, 0, c->stream, n, (const int64_t *)gp, (const int32_t *)gj, (const int32_t *)root, undec, stat);
        SPRS_HIP_TRY(c, hipGetLastError());
        SPRS_HIP_TRY(c, hipMemcpyAsync(h_stat, stat, sizeof(h_stat), hipMemcpyDeviceToHost, c->stream));
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (rounds > 0 && h_stat[1] == 0) {                  // (cannot happen: the largest undecided vertex wins its round)
            snprintf(c->err, sizeof(c->err), "sprs_amg: internal error: round %lld of the aggregation had no winner", (long long)rounds);
            return SPRS_ERR_HIP;
        }
        if (h_stat[0] == 0) break;
        if (rounds >= (int64_t)n) {
            snprintf(c->err, sizeof(c->err), "sprs_amg: internal error: %lld rounds left %u of %d vertices undecided", (long long)rounds, h_stat[0], n);
            return SPRS_ERR_HIP;
        }
        ++rounds;
        SPRS_HIP_TRY(c, hipMemsetAsync(stat, 0, sizeof(unsigned int) * 2, c->stream));
        hipLaunchKernelGGL(su_max_kernel, grid, block, 0, c->stream, n, seed, (const int64_t *)gp, (const int32_t *)gj, (const uint8_t *)undec, m1);
        hipLaunchKernelGGL(su_win_kernel, grid, block, 0, c->stream, n, seed, (const int64_t *)gp, (const int32_t *)gj, (const uint8_t *)undec, (const int32_t *)m1, root, stat);
    }
    SPRS_TRY(clk.lap(c, SG_ROUNDS));
    // pass 2, the numbering, T
    int h_bad = INT32_MAX;
    SPRS_HIP_TRY(c, hipMemcpyAsync(bad, &h_bad, sizeof(int), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL((su_pass2_kernel<R>), grid, block, 0, c->stream, n, (const int64_t *)gp, (const int32_t *)gj, (const R *)gw, (const int32_t *)root, root2, bad);
    hipLaunchKernelGGL(su_rootflag_kernel, grid1, block, 0, c->stream, n, (const int32_t *)root2, cnt);
    SPRS_HIP_TRY(c, rocprim::exclusive_scan(scratch, b32, cnt, m1, (int32_t)0, (size_t)n + 1, rocprim::plus<int32_t>(), c->stream));
    int32_t nc = 0;
    SPRS_HIP_TRY(c, hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipMemcpyAsync(&nc, m1 + n, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (h_bad != INT32_MAX) {                                // (cannot happen after a maximal pass 1: asserted, not assumed)
        snprintf(c->err, sizeof(c->err), "sprs_amg: internal error: pass 2 found no aggregated neighbour for row %d", h_bad);
        return SPRS_ERR_HIP;
    }
    hipLaunchKernelGGL((su_number_kernel<T>), grid1, block, 0, c->stream, n, (const int32_t *)root2, (const int32_t *)m1, agg, tip, tv);
    SPRS_HIP_TRY(c, hipGetLastError());
    SPRS_TRY(clk.lap(c, SG_PASS2));
    *nc_out = nc; *rounds_out = rounds;
    return SPRS_OK;
}

template <class T>
int amg_create_dev(const sprs_csr *A, double theta_d, int64_t coarse_max, int64_t max_levels, uint64_t seed, sprs_amg **out, int64_t *row_out) {
    using R = Real<T>;
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (A->nnz > (int64_t)INT32_MAX) {
        snprintf(c->err, sizeof(c->err), "sprs_amg: more than 2^31 - 1 stored entries");
        return SPRS_INVALID_ARGUMENT;
    }
    SPRS_TRY(sorted_columns_dev(A, "sprs_amg"));
    std::unique_ptr<sprs_amg, int (*)(sprs_amg *)> guard(new sprs_amg(), sprs_amg_destroy);   // freed on every early exit
    sprs_amg *P = guard.get();
    P->ctx = c; P->dtype = A->dtype; P->n = A->nrows; P->setup = 1;
    P->lv.reserve((size_t)AMG_MAX_LEVELS + 1);
    SetupClock clk(P->stage_ms);
    const R theta = (R)theta_d;
    DCsr<T> dA;                                              // the level's operator: level 0 reads the handle's own arrays
    dA.own = false; dA.n = dA.ncols = (int32_t)A->nrows; dA.nnz = A->nnz;
    dA.ip = A->row_ptr; dA.ix = A->col_idx; dA.v = (T *)A->val;
    while (true) {
        const int l = (int)P->lv.size();
        const int32_t n = dA.n;
        P->lv.emplace_back();
        AmgLevel &D = P->lv.back();
        D.n = n; D.nnz = dA.nnz;
        DevBufs tmp;
        R *md, *q, *rho;
        int *bad;
        char *scratch;
        SPRS_HIP_TRY(c, hipMalloc(&D.diag, sizeof(T) * ((size_t)n + 2)));
        SPRS_TRY(tmp.alloc(c, &md, (size_t)n));
        SPRS_TRY(tmp.alloc(c, &q, (size_t)n));
        SPRS_TRY(tmp.alloc(c, &rho, 1));
        SPRS_TRY(tmp.alloc(c, &bad, 1));
        int h_bad = INT32_MAX;
        R h_rho = R(1);
        SPRS_HIP_TRY(c, hipMemcpyAsync(bad, &h_bad, sizeof(int), hipMemcpyHostToDevice, c->stream));
        if (n) {
            hipLaunchKernelGGL((su_diag_kernel<T>), su_grid(n), dim3(BLOCK), 0, c->stream, (int)n, (const int32_t *)dA.ip, (const int32_t *)dA.ix, (const T *)dA.v,
                               (T *)D.diag, md, q, bad);
            SPRS_HIP_TRY(c, hipGetLastError());
            size_t bytes = 0;
            SPRS_HIP_TRY(c, rocprim::reduce(nullptr, bytes, q, rho, (size_t)n, NanMax{}, c->stream));
            SPRS_TRY(tmp.alloc(c, &scratch, bytes));
            SPRS_HIP_TRY(c, rocprim::reduce(scratch, bytes, q, rho, (size_t)n, NanMax{}, c->stream));
            SPRS_HIP_TRY(c, hipMemcpyAsync(&h_rho, rho, sizeof(R), hipMemcpyDeviceToHost, c->stream));
        }
        SPRS_HIP_TRY(c, hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (h_bad != INT32_MAX) { if (row_out) *row_out = h_bad; return SPRS_ZERO_DIAGONAL; }
        const R omega = R(4) / (R(3) * h_rho);
        D.omega = (double)omega;
        for (void **v : {&D.b, &D.x, &D.x2, &D.r}) SPRS_HIP_TRY(c, hipMalloc(v, sizeof(T) * ((size_t)n + 2)));
        SPRS_TRY(clk.lap(c, SG_DIAG));
        SPRS_TRY(su_pack<T>(c, D.A, n, dA.ip, dA.ix, dA.v));
        SPRS_TRY(clk.lap(c, SG_PACK));
        if (n <= coarse_max || l + 1 >= max_levels) break;
        // the aggregates (kept with the level: 4 bytes a row) and T
        DCsr<T> dT, dAT, dR, dAP, dAc;
        SPRS_HIP_TRY(c, hipMalloc((void **)&D.agg_dev, sizeof(int32_t) * ((size_t)n + 2)));
        dT.n = n; dT.nnz = n;
        SPRS_HIP_TRY(c, hipMalloc((void **)&dT.ip, sizeof(int32_t) * ((size_t)n + 2)));
        SPRS_HIP_TRY(c, hipMalloc((void **)&dT.v, sizeof(T) * ((size_t)n + 2)));
        int32_t nc = 0;
        SPRS_TRY(su_aggregate<T>(c, dA, md, (R)(theta * std::ldexp(R(1), -l)), seed, D.agg_dev, dT.ip, dT.v, &nc, &D.rounds, clk));
        if (2 * (int64_t)nc > n) {                           // the half-rows stop: this level is the coarsest
            (void)hipFree(D.agg_dev); D.agg_dev = nullptr; D.rounds = 0;
            break;
        }
        dT.ncols = nc; dT.ix = D.agg_dev;
        const int st_at = dev_product(c, dA, dT, dAT);
        dT.ix = nullptr;                                     // (the level's, not T's)
        SPRS_TRY(st_at);
        dT.reset();
        SPRS_TRY(clk.lap(c, SG_AT));
        hipLaunchKernelGGL((su_prolong_kernel<T>), su_grid(n), dim3(BLOCK), 0, c->stream, (int)n, (const int32_t *)dAT.ip, (const int32_t *)dAT.ix, dAT.v,
                           (const int32_t *)D.agg_dev, (const T *)D.diag, omega);
        SPRS_HIP_TRY(c, hipGetLastError());
        SPRS_TRY(clk.lap(c, SG_PROLONG));
        DCsr<T> &dP = dAT;                                   // P lives where A T was formed
        dR.n = nc; dR.ncols = n; dR.nnz = dP.nnz;
        SPRS_TRY(adjoint_dev<T>(c, "sprs_amg", n, nc, dP.nnz, dP.ip, dP.ix, dP.v, 1, &dR.ip, &dR.ix, &dR.v));
        SPRS_TRY(clk.lap(c, SG_ADJOINT));
        SPRS_TRY(dev_product(c, dA, dP, dAP));
        SPRS_TRY(clk.lap(c, SG_AP));
        SPRS_TRY(dev_product(c, dR, dAP, dAc));
        dAP.reset();
        SPRS_TRY(clk.lap(c, SG_RAP));
        D.pnnz = dP.nnz;
        SPRS_TRY(su_pack<T>(c, D.P, n, dP.ip, dP.ix, dP.v));
        SPRS_TRY(su_pack<T>(c, D.R, nc, dR.ip, dR.ix, dR.v));
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));    // (the fills read P and R, which go out of scope here)
        SPRS_TRY(clk.lap(c, SG_PACK));
        dA.take(dAc);
    }
    // the coarse solve: the coarsest operator comes down for the host's dense LU
    if (dA.n <= coarse_max) {
        HCsr<T> Ac;
        if (!to_host(dA, Ac)) return SPRS_ERR_HIP;
        std::vector<T> lu;
        const int64_t bad = dense_lu(Ac, lu);
        if (bad >= 0) { if (row_out) *row_out = bad; return SPRS_ZERO_DIAGONAL; }
        P->lu_n = Ac.n;
        T *dl = nullptr;
        const bool ok = dev_upload(&dl, lu.data(), lu.size());
        P->lu = dl;
        if (!ok) return SPRS_ERR_HIP;
    }
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));        // (the last fill reads dA)
    SPRS_TRY(clk.lap(c, SG_LU));
    SPRS_TRY(finish_handle<T>(P));
    *out = guard.release();
    return SPRS_OK;
}

// ---- sprs_amg_level_read on a device-built handle: the CSR arrays unpacked from the sliced-row layout on demand
int sell_unpack_host(sprs_ctx *c, const SellMat &M, size_t es, int32_t *row_ptr, int32_t *col_idx, void *val) {
    const size_t n = (size_t)M.n, nslice = (size_t)M.nslice;
    std::vector<int32_t> len(nslice * SELL_SLICE);
    std::vector<int64_t> sbase(nslice + 1);
    if (nslice) {
        SPRS_HIP_TRY(c, hipMemcpy(len.data(), M.len, sizeof(int32_t) * len.size(), hipMemcpyDeviceToHost));
        SPRS_HIP_TRY(c, hipMemcpy(sbase.data(), M.sbase, sizeof(int64_t) * sbase.size(), hipMemcpyDeviceToHost));
    }
    const size_t slots = nslice ? (size_t)sbase[nslice] : 0;
    std::vector<int32_t> col;
    std::vector<char> v;
    if (col_idx && slots) { col.resize(slots); SPRS_HIP_TRY(c, hipMemcpy(col.data(), M.col, sizeof(int32_t) * slots, hipMemcpyDeviceToHost)); }
    if (val && slots) { v.resize(slots * es); SPRS_HIP_TRY(c, hipMemcpy(v.data(), M.val, es * slots, hipMemcpyDeviceToHost)); }
    size_t at = 0;
    for (size_t p = 0; p < n; ++p) {
        if (row_ptr) row_ptr[p] = (int32_t)at;
        const size_t b = (size_t)sbase[p / SELL_SLICE] + p % SELL_SLICE;
        for (size_t e = 0; e < (size_t)len[p]; ++e, ++at) {
            if (col_idx && slots) col_idx[at] = col[b + e * SELL_SLICE];
            if (val && slots) memcpy((char *)val + at * es, v.data() + (b + e * SELL_SLICE) * es, es);
        }
    }
    if (row_ptr) row_ptr[n] = (int32_t)at;
    return SPRS_OK;
}

}  // namespace
