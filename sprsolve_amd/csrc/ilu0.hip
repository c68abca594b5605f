// ILU(0): the incomplete LU factorisation on A's own pattern, and the two triangular solves that apply it as a preconditioner
// (z = U^-1 (L^-1 r), L unit lower).  No reference analogue; the arithmetic is the serial loop stated in the header (sprs_ilu0_*).
//
// gs.hip's idea carries the whole file: rows are grouped into dependency levels (level(i) = 1 + max level(k) over the stored
// k < i; for the upper solve the same from the last row down), the rows of one level are independent, and ONE LANE folds ONE
// ROW left to right — so factors and solves are bit-identical to the serial loop for all four scalar types.  What gs.hip does
// not have:
//  * Level-major storage.  L's strictly-lower entries and U's strictly-upper entries (the pivots apart) are re-laid level by
//    level at creation in the sliced-row layout of sell.hpp: the rows of a level in ascending order at consecutive positions,
//    every level starting a new slice (a slice never spans two levels), so every value and column load is one coalesced
//    wavefront load instead of a walk through 64 scattered CSR rows.  A row is folded by sell.hpp's sell_fold, which skips
//    the padded slots.
//  * Small levels are batched.  A maximal run of consecutive levels of at most BLOCK rows each (at most ILU_MAX_BATCH_LEVELS of
//    them) is ONE launch of ONE workgroup that loops over the levels with __syncthreads() between them: the head and the tail
//    of a 3-D wavefront, every level of a 2-D grid, a tridiagonal matrix.  The vector being solved for is read and written
//    through plain pointers there, and the barrier orders one level's stores before the next level's loads (all wavefronts of
//    a workgroup share one CU and its L1).  A level of more than BLOCK rows is one launch of its own.  No kernel ever waits for
//    another workgroup: stream order between launches is the only inter-workgroup synchronisation.
// The factorisation runs on the same plan over a copy of A's values in CSR order (one lane per row, the row-k match by a
// two-pointer merge); the level-major copies are laid out from its result.
//
// A handle created with sweeps = k >= 1 (sprs_ilu0_create_sweeps) factorises in the same way and then replaces both exact
// solves by k Jacobi sweeps from the header's statement: one launch per sweep over the whole factor, whatever the level count.
// Such a handle keeps its factors in NATURAL row order and no level-major copy: the same layout with position = row, so a
// slice is full whatever the levels look like and neighbouring lanes gather neighbouring x.  A sweep reads the previous
// sweep's vector and writes another one (never in place), so its result does not depend on the launch geometry; the handle
// owns the three vectors the sweeps alternate between.
//
// An ORDERED handle (sprs_ilu0_create_ordered) is the exact handle of B = P A P^T: order.hip permutes A's arrays,
// the creation above runs on them unchanged, and the factor values go back to A's CSR positions for sprs_ilu0_read.  Its solves
// work in B's numbering on the handle's own y and apply P^T F^-1 P without a launch of their own: tri_row gathers its right-hand
// side at in[perm[row]] and stores its result at ext[perm[row]] as well (the ORD template flag; ORD_NONE is the natural path).
#include <algorithm>

#include "device.hpp"
#include "sell.hpp"

using namespace sprs;

namespace sprs {
constexpr int ILU_SLICE = SELL_SLICE;
// Levels per batched launch: bounds the run time of one kernel on a chain-like matrix (a level costs the one workgroup a few
// dependent memory round trips, some microseconds; 128 of them stay well below a millisecond).
constexpr int ILU_MAX_BATCH_LEVELS = 128;
}  // namespace sprs

namespace {

struct IluLaunch { int32_t l0, l1; bool batch; };   // levels [l0, l1): one workgroup looping over them, or (l1 == l0 + 1) one level

// runs of small levels -> one launch each, every larger level -> its own
std::vector<IluLaunch> make_plan(const std::vector<int32_t> &lvl_ptr) {
    std::vector<IluLaunch> plan;
    const int32_t nlev = (int32_t)lvl_ptr.size() - 1;
    for (int32_t l = 0; l < nlev; ++l) {
        const bool small = lvl_ptr[l + 1] - lvl_ptr[l] <= BLOCK;
        if (small && !plan.empty() && plan.back().batch && plan.back().l1 == l && l - plan.back().l0 < ILU_MAX_BATCH_LEVELS) plan.back().l1 = l + 1;
        else plan.push_back(IluLaunch{l, l + 1, small});
    }
    return plan;
}

// One triangular factor: level-major with its plan, or (a sweeps handle; lvl_slice, prow and the plan stay empty) in natural order.
struct IluTri {
    int32_t nlev = 0;
    std::vector<int32_t> h_lvl_slice;    // host: level l owns slices [h_lvl_slice[l], h_lvl_slice[l + 1])
    std::vector<IluLaunch> plan;
    SellMat M;                           // the strict triangle
    int32_t *lvl_slice = nullptr;        // device copy
    int32_t *prow = nullptr;             // device, per position: its row, -1 = no row
    void *piv = nullptr;                 // device, per position of T: u_ii (upper factor only)
    void release() {
        M.release();
        for (void *p : {(void *)lvl_slice, (void *)prow, piv}) if (p) (void)hipFree(p);
        lvl_slice = prow = nullptr; piv = nullptr;
    }
};

template <class T>
struct TriDev {
    const int32_t *lvl_slice, *prow;
    SellDev<T> M;
    const T *piv;
};

// One row by one lane: sigma over the row's entries in ascending column order, then the row's own element.  `in` and `out` may
// be the same vector; out[c] of an entry was written by an earlier level.
// ORD (an ordered handle; `out` is then a vector of the handle's, in the permuted numbering the factors are stored in):
// ORD_GATHER reads the row's right-hand side at in[perm[row]], ORD_SCATTER also stores the row's result at ext[perm[row]] — the
// two ends of P^T F^-1 P folded into the solves' own load and store.  `in` may be `ext`: a lane touches its own row's element only.
enum : int { ORD_NONE = 0, ORD_GATHER = 1, ORD_SCATTER = 2 };
template <class T>
struct OrdDev {
    const int32_t *perm;                 // new -> old
    T *ext;
};

template <class T, bool UPPER, int ORD>
__device__ __forceinline__ void tri_row(const TriDev<T> &F, int s, int t, const T *in, T *out, const OrdDev<T> &O) {
    const int p = s * ILU_SLICE + t;
    const int row = F.prow[p];
    if (row < 0) return;
    const T sigma = sell_fold<T>(F.M, p, out);
    const int old = ORD ? O.perm[row] : row;
    T d = ssub(in[(ORD & ORD_GATHER) ? old : row], sigma);           // (in[row] is loaded after the fold, not held across it)
    if (UPPER) d = sdiv(d, F.piv[p]);
    out[row] = d;
    if (ORD & ORD_SCATTER) O.ext[old] = d;
}

// a level of more than BLOCK rows: one wavefront per slice
template <class T, bool UPPER, int ORD>
__global__ __launch_bounds__(BLOCK) void tri_level_kernel(TriDev<T> F, int s0, int s1, const T *in, T *out, OrdDev<T> O) {
    const int s = s0 + (int)blockIdx.x * NWAVE + (int)(threadIdx.x >> 6);
    if (s < s1) tri_row<T, UPPER, ORD>(F, s, threadIdx.x & (WAVE - 1), in, out, O);
}

// levels [l0, l1) of at most BLOCK rows (NWAVE slices) each: one workgroup, a barrier between two levels
template <class T, bool UPPER, int ORD>
__global__ __launch_bounds__(BLOCK) void tri_batch_kernel(TriDev<T> F, int l0, int l1, const T *in, T *out, OrdDev<T> O) {
    const int w = threadIdx.x >> 6, t = threadIdx.x & (WAVE - 1);
    for (int l = l0; l < l1; ++l) {
        const int s = F.lvl_slice[l] + w;
        if (s < F.lvl_slice[l + 1]) tri_row<T, UPPER, ORD>(F, s, t, in, out, O);
        __syncthreads();
    }
}

// ---- Jacobi sweeps on a factor in natural row order (position = row)
template <class T>
struct SweepDev {
    SellDev<T> M;
    const T *piv;                        // u_ii per row (upper factor only)
};

// One sweep, one wavefront per slice: next_i = rhs_i - sigma_i(prev) for the lower factor, the same divided by u_ii for the
// upper one.  `prev` is never `next`; `rhs` may be `next` (a lane reads rhs of its own row only).
// FUSE (the last lower sweep of an application): the lane also stores the upper solve's first sweep, z1_i = next_i / u_ii.
template <class T, bool UPPER, bool FUSE>
__global__ __launch_bounds__(BLOCK) void sweep_kernel(SweepDev<T> F, int n, const T *rhs, const T *prev, T *next, const T *upiv, T *z1) {
    const int s = (int)blockIdx.x * NWAVE + (int)(threadIdx.x >> 6), t = threadIdx.x & (WAVE - 1);
    const int row = s * ILU_SLICE + t;
    if (row >= n) return;
    const T sigma = sell_fold<T>(F.M, row, prev);
    T d = ssub(rhs[row], sigma);
    if (UPPER) d = sdiv(d, F.piv[row]);
    next[row] = d;
    if (FUSE) z1[row] = sdiv(d, upiv[row]);
}

// the upper solve's first sweep on its own: out_i = in_i / u_ii (in may be out)
template <class T>
__global__ __launch_bounds__(BLOCK) void sweep_first_upper_kernel(int n, const T *in, const T *__restrict__ piv, T *out) {
    const int row = (int)blockIdx.x * BLOCK + (int)threadIdx.x;
    if (row < n) out[row] = sdiv(in[row], piv[row]);
}

// ---- the factorisation, in place on `a` (CSR order): row i by one lane
template <class T>
__device__ __forceinline__ void ilu_row(int i, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                        const int32_t *__restrict__ dpos, T *a) {
    const int end = rp[i + 1];
    for (int pk = rp[i]; pk < end; ++pk) {
        const int k = ci[pk];
        if (k >= i) break;
        const int dk = dpos[k];
        const T l = sdiv(a[pk], a[dk]);
        a[pk] = l;
        int q = dk + 1;
        const int qe = rp[k + 1];
        for (int pj = pk + 1; pj < end && q < qe;) {                 // columns j > k that rows i and k both store
            const int cj = ci[pj], cq = ci[q];
            if (cj == cq) { a[pj] = ssub(a[pj], smul(l, a[q])); ++pj; ++q; }
            else if (cj < cq) ++pj;
            else ++q;
        }
    }
}

template <class T>
__global__ __launch_bounds__(BLOCK) void ilu_level_kernel(int count, const int32_t *__restrict__ rows, const int32_t *__restrict__ rp,
                                                          const int32_t *__restrict__ ci, const int32_t *__restrict__ dpos, T *a) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < count) ilu_row<T>(rows[i], rp, ci, dpos, a);
}

template <class T>
__global__ __launch_bounds__(BLOCK) void ilu_batch_kernel(const int32_t *__restrict__ lvl_ptr, int l0, int l1, const int32_t *__restrict__ rows,
                                                          const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                          const int32_t *__restrict__ dpos, T *a) {
    for (int l = l0; l < l1; ++l) {
        const int i = lvl_ptr[l] + (int)threadIdx.x;
        if (i < lvl_ptr[l + 1]) ilu_row<T>(rows[i], rp, ci, dpos, a);
        __syncthreads();
    }
}

// smallest row whose pivot is exactly zero or not finite
template <class T>
__global__ __launch_bounds__(BLOCK) void ilu_pivot_check_kernel(int n, const int32_t *__restrict__ dpos, const T *__restrict__ a, int *__restrict__ bad) {
    for (int row = blockIdx.x * BLOCK + threadIdx.x; row < n; row += gridDim.x * BLOCK) {
        if (bad_pivot(a[dpos[row]])) atomicMin(bad, row);
    }
}

}  // namespace

struct sprs_ilu0 {
    sprs_ctx *ctx = nullptr;
    int dtype = 0;
    int64_t n = 0, nnz = 0;
    void *fval = nullptr;                // device, nnz of T: the factors at A's CSR positions (sprs_ilu0_read)
    IluTri L, U;
    void *ybuf = nullptr;                // device, n of T: y = L^-1 in of a which = 0 solve
    int sweeps = 0;                      // 0: exact level-scheduled solves; k >= 1: k Jacobi sweeps on natural-order factors
    void *sbuf[2] = {nullptr, nullptr};  // device, n of T each: with ybuf the vectors the sweeps alternate between (sweeps > 0)
    void *in_tmp = nullptr, *out_tmp = nullptr;   // staging of the host entry points (lazily allocated)
    // An ordered handle (sprs_ilu0_create_ordered): L, U and ybuf live in the numbering of B = P A P^T, fval and every vector that
    // goes in or comes out in A's.
    int32_t *perm = nullptr;             // device, n: row perm[p] of A is row p of B; null = natural order
    std::vector<int32_t> h_perm;
};

namespace {

template <class T>
TriDev<T> tri_dev(const IluTri &F) {
    return TriDev<T>{F.lvl_slice, F.prow, F.M.dev<T>(), (const T *)F.piv};
}

// out = F^-1 in: the launches of the factor's plan, asynchronous on the context's stream
template <class T, bool UPPER, int ORD = ORD_NONE>
int tri_solve(sprs_ctx *c, const IluTri &F, const T *in, T *out, OrdDev<T> O = OrdDev<T>{nullptr, nullptr}) {
    const TriDev<T> D = tri_dev<T>(F);
    for (const IluLaunch &p : F.plan) {
        if (p.batch) {
            hipLaunchKernelGGL((tri_batch_kernel<T, UPPER, ORD>), dim3(1), dim3(BLOCK), 0, c->stream, D, p.l0, p.l1, in, out, O);
        } else {
            const int s0 = F.h_lvl_slice[p.l0], s1 = F.h_lvl_slice[p.l1];
            hipLaunchKernelGGL((tri_level_kernel<T, UPPER, ORD>), dim3((s1 - s0 + NWAVE - 1) / NWAVE), dim3(BLOCK), 0, c->stream, D, s0, s1, in, out, O);
        }
    }
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

// An ordered handle's solves: P^T F^-1 P with the handle's y as the vector in the permuted numbering, no launch beyond the
// factors' plans.  An application gathers in its lower solve, runs the upper solve in place on y and scatters from it.
template <class T>
int ordered_apply(const sprs_ilu0 *P, int which, const T *in, T *out) {
    sprs_ctx *c = P->ctx;
    T *y = (T *)P->ybuf;
    const OrdDev<T> O{P->perm, out};
    if (which == 1) return tri_solve<T, false, ORD_GATHER | ORD_SCATTER>(c, P->L, in, y, O);
    if (which == 2) return tri_solve<T, true, ORD_GATHER | ORD_SCATTER>(c, P->U, in, y, O);
    SPRS_TRY((tri_solve<T, false, ORD_GATHER>(c, P->L, in, y, O)));
    return tri_solve<T, true, ORD_SCATTER>(c, P->U, (const T *)y, y, O);
}

// The k-sweep solves of the header on the stream: which = 1 costs k - 1 launches, which = 2 k, which = 0 2k - 2 (one for k = 1).
// Every sweep writes a vector that no lane of the launch reads as `prev`; only the last one writes `out`.
template <class T>
int sweeps_apply(const sprs_ilu0 *P, int which, const T *in, T *out) {
    sprs_ctx *c = P->ctx;
    const int n = (int)P->n, k = P->sweeps;
    if (!n) return SPRS_OK;
    const SweepDev<T> L{P->L.M.dev<T>(), nullptr}, U{P->U.M.dev<T>(), (const T *)P->U.piv};
    T *const buf[3] = {(T *)P->ybuf, (T *)P->sbuf[0], (T *)P->sbuf[1]};
    const dim3 grid((unsigned)((P->L.M.nslice + NWAVE - 1) / NWAVE)), egrid((unsigned)((n + BLOCK - 1) / BLOCK));
    const T *rhs = in;                   // the upper sweeps' right-hand side: y(k) of an application, `in` of which = 2
    T *spare = buf[0];                   // with buf[2] the two vectors the upper sweeps alternate between
    if (which != 2) {
        if (k == 1 && which == 1) {      // y(1) = in: no pass at all
            if (in != out) SPRS_HIP_TRY(c, hipMemcpyAsync(out, in, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
            return SPRS_OK;
        }
        const T *prev = in;              // y(1)
        if (which == 1 && k == 2 && in == out) {   // the only sweep would read y(1) where it writes: read a copy
            SPRS_HIP_TRY(c, hipMemcpyAsync(buf[2], in, sizeof(T) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
            prev = buf[2];
        }
        for (int m = 2; m <= k; ++m) {
            T *next = (m == k && which == 1) ? out : buf[m & 1];
            if (m == k && which == 0)
                hipLaunchKernelGGL((sweep_kernel<T, false, true>), grid, dim3(BLOCK), 0, c->stream, L, n, in, prev, next, U.piv, buf[2]);
            else
                hipLaunchKernelGGL((sweep_kernel<T, false, false>), grid, dim3(BLOCK), 0, c->stream, L, n, in, prev, next, (const T *)nullptr, (T *)nullptr);
            prev = next;
        }
        if (which == 1) { SPRS_HIP_TRY(c, hipGetLastError()); return SPRS_OK; }
        rhs = prev;                      // y(k): `in` itself for k = 1, else buf[k & 1]
        spare = buf[(k & 1) ^ 1];
    }
    if (k == 1 || which == 2)            // z(1) on its own; an application with k >= 2 has it in buf[2] from the fused launch
        hipLaunchKernelGGL((sweep_first_upper_kernel<T>), egrid, dim3(BLOCK), 0, c->stream, n, rhs, U.piv, k == 1 ? out : buf[2]);
    const T *prev = buf[2];
    for (int m = 2; m <= k; ++m) {
        T *next = m == k ? out : (prev == buf[2] ? spare : buf[2]);
        hipLaunchKernelGGL((sweep_kernel<T, true, false>), grid, dim3(BLOCK), 0, c->stream, U, n, rhs, prev, next, (const T *)nullptr, (T *)nullptr);
        prev = next;
    }
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

// Host side of one factor: its packed strict triangle and (the upper factor) u_ii per position, ones where no row is.
template <class T>
struct TriHost {
    SellPacked<T> S;
    std::vector<T> piv;
};

// The row of every position from row_of (-1: none), row i's entries the CSR positions [eb(i), ee(i)) of ci / fv (the factorised
// values); dpos: the diagonal's positions (the upper factor), or null.  The pivots are gathered in the packer's own pass.
template <class T, class ROW, class EB, class EE>
TriHost<T> pack_tri(int64_t npos, ROW row_of, const std::vector<int32_t> &ci, const std::vector<T> &fv, EB eb, EE ee, const std::vector<int32_t> *dpos) {
    TriHost<T> H;
    if (!dpos) { H.S = sell_pack<T>(npos, row_of, eb, ee, ci.data(), fv.data()); return H; }
    H.piv.assign((size_t)(npos + ILU_SLICE - 1) / ILU_SLICE * ILU_SLICE, sone<T>());
    H.S = sell_pack<T>(npos, row_of, eb, ee, ci.data(), fv.data(), [&](size_t p, int32_t i) { H.piv[p] = fv[(size_t)(*dpos)[(size_t)i]]; });
    return H;
}

template <class T>
int upload_tri(IluTri &F, int64_t npos, const TriHost<T> &H) {
    T *dpiv = nullptr;
    const bool ok = F.M.upload(npos, H.S) && (H.piv.empty() || dev_upload(&dpiv, H.piv.data(), H.piv.size()));
    F.piv = dpiv;
    return ok ? SPRS_OK : SPRS_ERR_HIP;
}

// Level-major layout of one factor: the rows of level l at the positions from slice h_lvl_slice[l] on, and the launch plan.
// All host work first, then the uploads.
template <class T, class EB, class EE>
int build_tri(IluTri &F, const std::vector<int32_t> &lvl_ptr, const std::vector<int32_t> &rows, const std::vector<int32_t> &ci,
              const std::vector<T> &fv, EB eb, EE ee, const std::vector<int32_t> *dpos) {
    const int32_t nlev = (int32_t)lvl_ptr.size() - 1;
    F.h_lvl_slice.assign((size_t)nlev + 1, 0);
    for (int32_t l = 0; l < nlev; ++l) F.h_lvl_slice[l + 1] = F.h_lvl_slice[l] + (lvl_ptr[l + 1] - lvl_ptr[l] + ILU_SLICE - 1) / ILU_SLICE;
    F.plan = make_plan(lvl_ptr);
    std::vector<int32_t> prow((size_t)F.h_lvl_slice[nlev] * ILU_SLICE, -1);
    for (int32_t l = 0; l < nlev; ++l)
        std::copy(rows.begin() + lvl_ptr[l], rows.begin() + lvl_ptr[l + 1], prow.begin() + (size_t)F.h_lvl_slice[l] * ILU_SLICE);
    const TriHost<T> H = pack_tri<T>((int64_t)prow.size(), [&](size_t p) { return prow[p]; }, ci, fv, eb, ee, dpos);
    if (!dev_upload(&F.lvl_slice, F.h_lvl_slice.data(), F.h_lvl_slice.size()) || !dev_upload(&F.prow, prow.data(), prow.size())) return SPRS_ERR_HIP;
    return upload_tri<T>(F, (int64_t)prow.size(), H);
}

template <class T>
int ilu0_create(const CsrView &A, int sweeps, sprs_ilu0 **out, int64_t *row_out) {
    sprs_ctx *c = A.ctx;
    CtxLock lock(c);
    const int64_t n = A.nrows, nnz = A.nnz;
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    // the pattern on the host: its checks, the diagonal positions and both level rules
    std::vector<int32_t> rp, ci;
    SPRS_TRY(host_pattern(A, "sprs_ilu0", rp, ci));
    std::vector<int32_t> dpos((size_t)n, -1);
    for (int64_t i = 0; i < n; ++i) {
        dpos[i] = (int32_t)diag_pos(rp.data(), ci.data(), i);
        if (dpos[i] < 0) { if (row_out) *row_out = i; return SPRS_ZERO_DIAGONAL; }
    }
    std::vector<int32_t> level((size_t)n, 0), ulevel((size_t)n, 0);
    int32_t nlev = n ? 1 : 0, nulev = n ? 1 : 0;
    for (int64_t i = 0; i < n; ++i) {
        int32_t l = 0;
        for (int32_t k = rp[i]; k < dpos[i]; ++k) l = std::max(l, level[ci[k]] + 1);
        level[i] = l; nlev = std::max(nlev, l + 1);
    }
    for (int64_t i = n - 1; i >= 0; --i) {
        int32_t l = 0;
        for (int32_t k = dpos[i] + 1; k < rp[i + 1]; ++k) l = std::max(l, ulevel[ci[k]] + 1);
        ulevel[i] = l; nulev = std::max(nulev, l + 1);
    }
    std::vector<int32_t> lptr, lrows, uptr, urows;
    group_by_level(level, nlev, lptr, lrows);
    group_by_level(ulevel, nulev, uptr, urows);

    auto *P = new sprs_ilu0();
    P->ctx = c; P->dtype = A.dtype; P->n = n; P->nnz = nnz; P->sweeps = sweeps;
    int32_t *d_dpos = nullptr, *d_rows = nullptr, *d_lptr = nullptr;
    int *d_bad = nullptr;
    auto fail = [&](int st) {
        for (void *p : {(void *)d_dpos, (void *)d_rows, (void *)d_lptr, (void *)d_bad}) if (p) (void)hipFree(p);
        sprs_ilu0_destroy(P);
        return st;
    };
    T *a = nullptr;
    if (hipMalloc((void **)&a, sizeof(T) * ((size_t)nnz + 2)) != hipSuccess) return fail(SPRS_ERR_HIP);
    P->fval = a;
    if (hipMalloc(&P->ybuf, sizeof(T) * ((size_t)n + 2)) != hipSuccess) return fail(SPRS_ERR_HIP);
    for (void *&b : P->sbuf) if (sweeps && hipMalloc(&b, sizeof(T) * ((size_t)n + 2)) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (!dev_upload(&d_dpos, dpos.data(), dpos.size()) || !dev_upload(&d_rows, lrows.data(), lrows.size()) ||
        !dev_upload(&d_lptr, lptr.data(), lptr.size()) || hipMalloc((void **)&d_bad, sizeof(int)) != hipSuccess) return fail(SPRS_ERR_HIP);
    int bad = INT32_MAX;
    if ((nnz && hipMemcpyAsync(a, A.val, sizeof(T) * (size_t)nnz, hipMemcpyDeviceToDevice, c->stream) != hipSuccess) ||
        hipMemcpyAsync(d_bad, &bad, sizeof(int), hipMemcpyHostToDevice, c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
    // the factorisation: level by level, on the lower solve's plan
    for (const IluLaunch &p : make_plan(lptr)) {
        if (p.batch) hipLaunchKernelGGL((ilu_batch_kernel<T>), dim3(1), dim3(BLOCK), 0, c->stream, d_lptr, p.l0, p.l1, d_rows, A.row_ptr, A.col_idx, d_dpos, a);
        else {
            const int cnt = lptr[p.l1] - lptr[p.l0];
            hipLaunchKernelGGL((ilu_level_kernel<T>), dim3((cnt + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream, cnt, d_rows + lptr[p.l0], A.row_ptr, A.col_idx, d_dpos, a);
        }
    }
    if (n) hipLaunchKernelGGL((ilu_pivot_check_kernel<T>), dim3((int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 2048)), dim3(BLOCK), 0, c->stream,
                              (int)n, d_dpos, a, d_bad);
    std::vector<T> fv((size_t)nnz);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        (nnz && hipMemcpyAsync(fv.data(), a, sizeof(T) * (size_t)nnz, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        hipStreamSynchronize(c->stream) != hipSuccess) {
        snprintf(c->err, sizeof(c->err), "sprs_ilu0: the factorisation failed on the device (%s)", hipGetErrorString(hipGetLastError()));
        return fail(SPRS_ERR_HIP);
    }
    if (bad != INT32_MAX) { if (row_out) *row_out = bad; return fail(SPRS_ZERO_DIAGONAL); }
    // the level-major copies of both factors, or (a sweeps handle) the natural-order ones in their place: position = row, and
    // the level counts for sprs_ilu0_levels only
    auto lb = [&](int32_t i) { return rp[i]; }; auto le = [&](int32_t i) { return dpos[i]; };
    auto ub = [&](int32_t i) { return dpos[i] + 1; }; auto ue = [&](int32_t i) { return rp[i + 1]; };
    auto natural = [](size_t p) { return (int32_t)p; };
    P->L.nlev = nlev; P->U.nlev = nulev;
    int st = sweeps ? upload_tri<T>(P->L, n, pack_tri<T>(n, natural, ci, fv, lb, le, nullptr)) : build_tri<T>(P->L, lptr, lrows, ci, fv, lb, le, nullptr);
    if (st == SPRS_OK) st = sweeps ? upload_tri<T>(P->U, n, pack_tri<T>(n, natural, ci, fv, ub, ue, &dpos)) : build_tri<T>(P->U, uptr, urows, ci, fv, ub, ue, &dpos);
    if (st != SPRS_OK) return fail(st);
    for (void *p : {(void *)d_dpos, (void *)d_rows, (void *)d_lptr, (void *)d_bad}) (void)hipFree(p);
    *out = P;
    return SPRS_OK;
}

// the factor values of B's entries at the positions of A's arrays they came from
template <class T>
__global__ __launch_bounds__(BLOCK) void ilu_unpermute_kernel(int64_t nnz, const int32_t *__restrict__ src, const T *__restrict__ fb, T *__restrict__ fa) {
    for (int64_t q = (int64_t)blockIdx.x * BLOCK + threadIdx.x; q < nnz; q += (int64_t)gridDim.x * BLOCK) fa[src[q]] = fb[q];
}

// The ordered handle: the exact handle of B = P A P^T (built here on raw arrays, no operator handle), its factor values moved
// back to A's positions, and the permutation for the solves.  perm: a checked permutation.
template <class T>
int ilu0_create_ordered(const sprs_csr *A, std::vector<int32_t> perm, sprs_ilu0 **out, int64_t *row_out) {
    sprs_ctx *c = A->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    const int64_t n = A->nrows, nnz = A->nnz;
    SPRS_TRY(sorted_columns_dev(A, "sprs_ilu0"));   // (the permutation ranks a row's columns: they must be distinct)
    DevBufs tmp;
    int32_t *d_perm, *rp = nullptr, *ci = nullptr, *src = nullptr;
    void *val = nullptr;
    T *fa;
    SPRS_TRY(tmp.alloc(c, &d_perm, (size_t)n + 2));
    SPRS_TRY(tmp.alloc(c, &fa, (size_t)nnz + 2));
    if (n) SPRS_HIP_TRY(c, hipMemcpyAsync(d_perm, perm.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    SPRS_TRY(csr_permute_arrays(A, d_perm, &rp, &ci, &val, &src));
    tmp.p.push_back(rp); tmp.p.push_back(ci); tmp.p.push_back(val); tmp.p.push_back(src);
    const CsrView B{c, A->dtype, n, n, nnz, rp, ci, val};
    sprs_ilu0 *P = nullptr;
    int64_t row = -1;
    const int st = ilu0_create<T>(B, 0, &P, &row);
    if (st == SPRS_ZERO_DIAGONAL && row_out && row >= 0) *row_out = perm[(size_t)row];
    SPRS_TRY(st);
    if (nnz) {
        hipLaunchKernelGGL((ilu_unpermute_kernel<T>), dim3((unsigned)std::min<int64_t>((nnz + BLOCK - 1) / BLOCK, 4 * (int64_t)grid_for(c))), dim3(BLOCK), 0, c->stream,
                           nnz, src, (const T *)P->fval, fa);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
            sprs_ilu0_destroy(P);
            snprintf(c->err, sizeof(c->err), "sprs_ilu0: moving the factors to A's positions failed on the device");
            return SPRS_ERR_HIP;
        }
    }
    (void)hipFree(P->fval);
    P->fval = fa; tmp.release(fa);
    P->perm = d_perm; tmp.release(d_perm);
    P->h_perm = std::move(perm);
    *out = P;
    return SPRS_OK;
}

template <class T>
int ilu0_solve_host(const sprs_ilu0 *Pc, int which, const T *in, size_t in_len, T *out, size_t out_len) {
    if (!Pc || !in || !out || Pc->dtype != dtype_of<T>::value || which < 0 || which > 2) return SPRS_INVALID_ARGUMENT;
    if (in_len != (size_t)Pc->n || out_len != (size_t)Pc->n) return SPRS_DIM_MISMATCH;
    return staged_apply<T>(Pc, in, out, [&](const T *din, T *dout) { return ilu0_apply<T>(Pc, which, din, dout); });
}

}  // namespace

namespace sprs {

int ilu0_check(const sprs_ilu0 *P, const sprs_csr *A, int dtype, size_t n) { return applied_check(P, A, dtype, n); }

template <class T>
int ilu0_apply(const sprs_ilu0 *P, int which, const T *in, T *out) {
    if (!P || !in || !out || P->dtype != dtype_of<T>::value || which < 0 || which > 2) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = P->ctx;
    CtxLock lock(c);   // ybuf is per-handle scratch
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (P->sweeps) return sweeps_apply<T>(P, which, in, out);
    if (P->perm) return ordered_apply<T>(P, which, in, out);
    if (which == 1) return tri_solve<T, false>(c, P->L, in, out);
    if (which == 2) return tri_solve<T, true>(c, P->U, in, out);
    SPRS_TRY((tri_solve<T, false>(c, P->L, in, (T *)P->ybuf)));
    return tri_solve<T, true>(c, P->U, (const T *)P->ybuf, out);
}
template int ilu0_apply<double>(const sprs_ilu0 *, int, const double *, double *);
template int ilu0_apply<cplx>(const sprs_ilu0 *, int, const cplx *, cplx *);
template int ilu0_apply<float>(const sprs_ilu0 *, int, const float *, float *);
template int ilu0_apply<cplxf>(const sprs_ilu0 *, int, const cplxf *, cplxf *);

template <class T>
AppliedPrec<T> ilu0_prec(const sprs_ilu0 *P) {
    return AppliedPrec<T>{P, [](const void *h, const sprs_csr *A, int dtype, size_t n) { return ilu0_check((const sprs_ilu0 *)h, A, dtype, n); },
                          [](const void *h, const T *in, T *out) { return ilu0_apply<T>((const sprs_ilu0 *)h, 0, in, out); }};
}
template AppliedPrec<double> ilu0_prec<double>(const sprs_ilu0 *);
template AppliedPrec<cplx> ilu0_prec<cplx>(const sprs_ilu0 *);
template AppliedPrec<float> ilu0_prec<float>(const sprs_ilu0 *);
template AppliedPrec<cplxf> ilu0_prec<cplxf>(const sprs_ilu0 *);

}  // namespace sprs

#define SPRS_G(...) try { __VA_ARGS__ } catch (...) { return SPRS_ERR_HIP; }

extern "C" {

int sprs_ilu0_create_sweeps(const sprs_csr *A, int sweeps, sprs_ilu0 **out, int64_t *row_out) {
    SPRS_G(
        if (!A || !out) return SPRS_INVALID_ARGUMENT;
        *out = nullptr;
        if (row_out) *row_out = -1;
        SPRS_TRY(single_gpu_only(A, "sprs_ilu0"));   // (before the shape: a row block with a halo has more columns than rows)
        if (sweeps < 0 || sweeps > SPRS_ILU0_MAX_SWEEPS) {
            snprintf(A->ctx->err, sizeof(A->ctx->err), "sprs_ilu0: sweeps must be in 0 .. %d (0 = exact solves), got %d", SPRS_ILU0_MAX_SWEEPS, sweeps);
            return SPRS_INVALID_ARGUMENT;
        }
        if (A->nrows != A->ncols) return SPRS_NOT_SQUARE;
        switch (A->dtype) {
            case DT_D: return ilu0_create<double>(csr_view(A), sweeps, out, row_out);
            case DT_Z: return ilu0_create<cplx>(csr_view(A), sweeps, out, row_out);
            case DT_S: return ilu0_create<float>(csr_view(A), sweeps, out, row_out);
            case DT_C: return ilu0_create<cplxf>(csr_view(A), sweeps, out, row_out);
        }
        return SPRS_INVALID_ARGUMENT;)
}

int sprs_ilu0_create(const sprs_csr *A, sprs_ilu0 **out, int64_t *row_out) { return sprs_ilu0_create_sweeps(A, 0, out, row_out); }

int sprs_ilu0_sweeps(const sprs_ilu0 *P) { return P ? P->sweeps : -1; }

int sprs_ilu0_create_ordered(const sprs_csr *A, int sweeps, int order, const int32_t *perm_host, size_t perm_len, sprs_ilu0 **out, int64_t *row_out) {
    if (order == SPRS_ORDER_NATURAL) return sprs_ilu0_create_sweeps(A, sweeps, out, row_out);
    SPRS_G(
        if (!A || !out) return SPRS_INVALID_ARGUMENT;
        *out = nullptr;
        if (row_out) *row_out = -1;
        SPRS_TRY(single_gpu_only(A, "sprs_ilu0"));
        if (order != SPRS_ORDER_MULTICOLOR && order != SPRS_ORDER_PERM) return refuse(A->ctx, "sprs_ilu0", "order must be SPRS_ORDER_NATURAL, _MULTICOLOR or _PERM, got %d", order);
        if (sweeps != 0) return refuse(A->ctx, "sprs_ilu0", "an ordering takes exact solves only (sweeps = 0), got sweeps = %d: with few levels the sweeps have no purpose", sweeps);
        if (A->nrows != A->ncols) return SPRS_NOT_SQUARE;
        std::vector<int32_t> perm;
        if (order == SPRS_ORDER_MULTICOLOR) {
            std::vector<int32_t> colors;
            int64_t ncolors = 0;
            SPRS_TRY(csr_color_host(A, 0, colors, &ncolors, nullptr));
            perm = color_major_perm(colors, ncolors);
        } else {
            if (!perm_host && perm_len) return SPRS_INVALID_ARGUMENT;
            SPRS_TRY(perm_check(A->ctx, "sprs_ilu0", perm_host, perm_len, A->nrows));
            perm.assign(perm_host, perm_host + perm_len);
        }
        switch (A->dtype) {
            case DT_D: return ilu0_create_ordered<double>(A, std::move(perm), out, row_out);
            case DT_Z: return ilu0_create_ordered<cplx>(A, std::move(perm), out, row_out);
            case DT_S: return ilu0_create_ordered<float>(A, std::move(perm), out, row_out);
            case DT_C: return ilu0_create_ordered<cplxf>(A, std::move(perm), out, row_out);
        }
        return SPRS_INVALID_ARGUMENT;)
}

int sprs_ilu0_order(const sprs_ilu0 *P, int32_t *perm_host) {
    if (!P) return -1;
    if (!P->perm) return 0;
    if (perm_host) std::copy(P->h_perm.begin(), P->h_perm.end(), perm_host);
    return 1;
}

int sprs_ilu0_destroy(sprs_ilu0 *P) {
    if (!P) return SPRS_OK;
    if (P->ctx) { (void)hipSetDevice(P->ctx->device); (void)hipStreamSynchronize(P->ctx->stream); }
    P->L.release(); P->U.release();
    for (void *p : {P->fval, P->ybuf, P->sbuf[0], P->sbuf[1], P->in_tmp, P->out_tmp, (void *)P->perm}) if (p) (void)hipFree(p);
    delete P;
    return SPRS_OK;
}

int sprs_ilu0_levels(const sprs_ilu0 *P, int64_t *lower_levels, int64_t *upper_levels, int64_t *lower_launches, int64_t *upper_launches) {
    if (!P) return SPRS_INVALID_ARGUMENT;
    if (lower_levels) *lower_levels = P->L.nlev;
    if (upper_levels) *upper_levels = P->U.nlev;
    if (lower_launches) *lower_launches = P->sweeps ? P->sweeps - 1 : (int64_t)P->L.plan.size();
    if (upper_launches) *upper_launches = P->sweeps ? P->sweeps : (int64_t)P->U.plan.size();
    return SPRS_OK;
}

int sprs_ilu0_read(const sprs_ilu0 *P, void *val_host) {
    if (!P || (!val_host && P->nnz)) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = P->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (P->nnz) SPRS_HIP_TRY(c, hipMemcpyAsync(val_host, P->fval, dtype_size(P->dtype) * (size_t)P->nnz, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

#define SPRS_ILU_API(X, T, CT)                                                                                          \
    int sprs_ilu0_solve_dev_##X(const sprs_ilu0 *P, int which, const CT *in, CT *out) {                                 \
        SPRS_G(return ilu0_apply<T>(P, which, (const T *)in, (T *)out);)                                                \
    }                                                                                                                   \
    int sprs_ilu0_solve_##X(const sprs_ilu0 *P, int which, const CT *in, size_t il, CT *out, size_t ol) {               \
        SPRS_G(return ilu0_solve_host<T>(P, which, (const T *)in, il, (T *)out, ol);)                                   \
    }
SPRS_ILU_API(d, double, double)
SPRS_ILU_API(z, cplx, sprs_c64)
SPRS_ILU_API(s, float, float)
SPRS_ILU_API(c, cplxf, sprs_c32)

}  // extern "C"
