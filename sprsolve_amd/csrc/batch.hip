// On-chip batch solvers: nbatch small systems that share one CSR pattern, one workgroup per system, one launch per call.  No
// reference analogue; the arithmetic is the statement in the header (sprs_batch_*), the plan is batch_plan.hpp, DESIGN.md §4u.
//
//  * Layout.  The pattern is kept once in the 64-row sliced, slice-column-major layout of sell.hpp (position = row): len per row,
//    sbase per slice, col per slot.  Every system's values are kept in the same layout, `slots` scalars per system one after
//    another, so lane t of a wavefront reads entry e of its row next to its neighbours' — every matrix load is one coalesced
//    wavefront load — and the row fold is sell_fold(), the one ILU(0) and AMG apply their operators with.  The slots a shorter
//    row leaves are zero and are skipped, never multiplied.  dst[k] is the slot of CSR entry k: set_values scatters through it,
//    read gathers through it.  dslot[i] is the slot of row i's diagonal entry (-1: not stored).
//  * Solve kernels (batch_bicgstab_kernel, batch_cg_kernel).  Workgroup b owns system b: B(n) threads, thread t owns the rows
//    t, t + B, ..  Every vector of the recurrence lives in dynamic LDS behind 128 bytes of reduction scratch; element-wise
//    statements touch owned rows only, so they need no barrier; a product A u is fenced by a barrier before (u is complete) and
//    after (nobody overwrites u while a neighbour still gathers from it); a sum over rows is wg_sum(): strided partials, the
//    wavefront butterfly, the wavefronts left to right — every thread returns the same bits, so every branch on a scalar is
//    uniform and a system that stops leaves its loop as a whole workgroup.  No workgroup reads what another writes; every loop is
//    bounded by max_iter or n; there is no spin wait.  rhs is read from HBM where the recurrence reads it; x and the three result
//    words are written once, at the end.
#include <numeric>

#include "device.hpp"
#include "sell.hpp"
#include "batch_plan.hpp"

using namespace sprs;

static_assert((int)BATCH_BICGSTAB == (int)SPRS_BATCH_BICGSTAB && (int)BATCH_CG == (int)SPRS_BATCH_CG, "the plan's solver codes are the header's");
static_assert(BATCH_WAVE == WAVE && BATCH_MAX_THREADS == BLOCK, "the plan's wavefront and workgroup are the library's");
static_assert((int)DT_D == 0 && (int)DT_Z == 1 && (int)DT_S == 2 && (int)DT_C == 3, "batch_scalar_bytes() takes the handles' dtype codes");

struct sprs_batch {
    sprs_ctx *ctx = nullptr;
    int dtype = 0;
    int64_t n = 0, nnz = 0, nbatch = 0, slots = 0;
    int64_t nodiag_row = -1;                      // the smallest row that stores no diagonal entry (-1: every row does)
    int32_t *len = nullptr, *col = nullptr;       // device: the pattern, packed
    int64_t *sbase = nullptr;
    int32_t *dst = nullptr, *dslot = nullptr;     // device: slot of CSR entry k; slot of row i's diagonal entry
    void *val = nullptr;                          // device: nbatch * slots of T
    unsigned long long *d_its = nullptr;          // device, nbatch each: what the solve kernels report
    void *d_res = nullptr;
    int *d_status = nullptr;
    void *a_tmp = nullptr, *b_tmp = nullptr;      // staging of the host entry points: nbatch * n of T each (lazily allocated)
};

namespace {

// ---- values in and out of the packed layout
template <class T>
__global__ __launch_bounds__(BLOCK) void batch_scatter_kernel(int64_t total, int64_t nnz, int64_t slots, const int32_t *__restrict__ dst,
                                                              const T *__restrict__ values, T *__restrict__ val) {
    for (int64_t idx = (int64_t)blockIdx.x * BLOCK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * BLOCK) {
        const int64_t b = idx / nnz, k = idx - b * nnz;
        val[b * slots + dst[k]] = values[idx];
    }
}
template <class T>
__global__ __launch_bounds__(BLOCK) void batch_gather_kernel(int64_t total, int64_t nnz, int64_t slots, const int32_t *__restrict__ dst,
                                                             const T *__restrict__ val, T *__restrict__ values) {
    for (int64_t idx = (int64_t)blockIdx.x * BLOCK + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * BLOCK) {
        const int64_t b = idx / nnz, k = idx - b * nnz;
        values[idx] = val[b * slots + dst[k]];
    }
}

// what every kernel of a batch is given
template <class T>
struct BatchDev {
    const int32_t *len;
    const int64_t *sbase;
    const int32_t *col;
    const T *val;                // system b's values start at val + b * slots
    const int32_t *dslot;
    int64_t slots;
    int n;
    __device__ __forceinline__ SellDev<T> system(int64_t b) const { return SellDev<T>{len, sbase, col, val + b * slots}; }
};

// y_b = A_b x_b, x and y in HBM: workgroup b, thread t the rows t, t + B, ..
template <class T>
__global__ __launch_bounds__(BLOCK) void batch_mul_vec_kernel(BatchDev<T> D, const T *__restrict__ x, T *__restrict__ y) {
    const int64_t b = blockIdx.x;
    const SellDev<T> M = D.system(b);
    const T *xb = x + b * D.n;
    T *yb = y + b * D.n;
    for (int i = (int)threadIdx.x; i < D.n; i += (int)blockDim.x) yb[i] = sell_fold(M, i, xb);
}

// ---- sums over the workgroup in the statement's order; every thread returns the same bits.  `scr`: BATCH_SCRATCH bytes.
template <class S>
__device__ __forceinline__ S wg_sum(S v, unsigned char *scr) {
    v = wave_sum(v);
    S *red = reinterpret_cast<S *>(scr);
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();             // the previous sum's readers are done
    if (lane == 0) red[wv] = v;
    __syncthreads();
    S acc = red[0];
    for (int w = 1; w < nw; ++w) acc = sadd(acc, red[w]);
    return acc;
}
// two sums that share their barriers: the bits of two wg_sum calls
template <class SA, class SB>
__device__ __forceinline__ void wg_sum2(SA a, SB b, unsigned char *scr, SA &ra, SB &rb) {
    a = wave_sum(a); b = wave_sum(b);
    SA *redA = reinterpret_cast<SA *>(scr);
    SB *redB = reinterpret_cast<SB *>(scr + BATCH_SCRATCH / 2);
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) { redA[wv] = a; redB[wv] = b; }
    __syncthreads();
    ra = redA[0]; rb = redB[0];
    for (int w = 1; w < nw; ++w) { ra = sadd(ra, redA[w]); rb = sadd(rb, redB[w]); }
}

#define BATCH_EACH(i) for (int i = tid; i < n; i += nthr)

// out = A in on LDS vectors (in != out)
template <class T>
__device__ __forceinline__ void wg_spmv(const SellDev<T> &M, const T *in, T *out, int n, int tid, int nthr) {
    __syncthreads();
    BATCH_EACH(i) out[i] = sell_fold(M, i, in);
    __syncthreads();
}
template <class T>
__device__ __forceinline__ Real<T> wg_norm2(const T *a, int n, int tid, int nthr, unsigned char *scr) {
    Real<T> s = 0;
    BATCH_EACH(i) s = s + ssq(a[i]);
    return ssqrt(wg_sum(s, scr));
}
template <class T>
__device__ __forceinline__ T wg_cdot(const T *a, const T *b, int n, int tid, int nthr, unsigned char *scr) {
    T s = szero<T>();
    BATCH_EACH(i) s = sadd(s, smul(sconj(a[i]), b[i]));
    return wg_sum(s, scr);
}

template <class T>
struct BatchSolveArgs {
    BatchDev<T> D;
    const T *rhs;
    T *x;
    unsigned long long max_iter;
    Real<T> tol;
    unsigned long long *its;
    Real<T> *res;
    int *status;
};

// x to HBM and the three result words: the end of every path through a solve kernel
template <class T>
__device__ __forceinline__ void batch_finish(const BatchSolveArgs<T> &a, int64_t b, const T *x, T *xg, int n, int tid, int nthr, int st,
                                             unsigned long long its, Real<T> res) {
    BATCH_EACH(i) xg[i] = x[i];
    if (tid == 0) { a.its[b] = its; a.res[b] = res; a.status[b] = st; }
}

// BiCGStab per system: the recurrence of sprs_bicgstab_solve_* (PC = false) / sprs_bicgstab_precond_solve_* with
// dinv_i = one / a_ii (PC = true), statement for statement.
template <class T, bool PC>
__global__ __launch_bounds__(BLOCK) void batch_bicgstab_kernel(BatchSolveArgs<T> a) {
    using R = Real<T>;
    const int n = a.D.n, tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int64_t b = blockIdx.x;
    const SellDev<T> M = a.D.system(b);
    extern __shared__ __align__(16) unsigned char batch_lds[];   // all of it dynamic: the carve offsets stay multiples of 16
    unsigned char *scr = batch_lds;
    T *vec = reinterpret_cast<T *>(batch_lds + BATCH_SCRATCH);
    T *x = vec, *r = vec + n, *r0 = vec + 2 * (size_t)n, *y = vec + 3 * (size_t)n, *p = vec + 4 * (size_t)n, *v = vec + 5 * (size_t)n,
      *t = vec + 6 * (size_t)n, *z = vec + 7 * (size_t)n;
    const T *rhs = a.rhs + b * n;
    T *xg = a.x + b * n;
    const R eps = seps<R>();
    const T one = sone<T>(), mone = sneg(sone<T>());
    auto dinv = [&](int i) { return sdiv(one, M.val[a.D.dslot[i]]); };

    const R rhs_norm = wg_norm2(rhs, n, tid, nthr, scr);
    if (rhs_norm <= eps) {
        BATCH_EACH(i) xg[i] = szero<T>();
        if (tid == 0) { a.its[b] = 0; a.res[b] = rhs_norm; a.status[b] = SPRS_OK; }
        return;
    }
    const R tol2 = a.tol * rhs_norm;
    BATCH_EACH(i) x[i] = xg[i];
    wg_spmv(M, x, r, n, tid, nthr);
    BATCH_EACH(i) { r[i] = sadd(r[i], smul(rhs[i], mone)); r0[i] = r[i]; }
    const R r0_norm = wg_norm2(r0, n, tid, nthr, scr);
    if (r0_norm <= tol2) { batch_finish(a, b, x, xg, n, tid, nthr, SPRS_OK, 0, r0_norm / rhs_norm); return; }
    R r0_norm_tol = r0_norm * eps;
    r0_norm_tol = r0_norm_tol * r0_norm_tol;
    T rho = sfromr<T>(r0_norm * r0_norm);
    if (PC) { BATCH_EACH(i) { p[i] = r[i]; y[i] = smul(p[i], dinv(i)); } }
    else { BATCH_EACH(i) y[i] = r[i]; }
    wg_spmv(M, y, v, n, tid, nthr);
    T alpha = sdiv(rho, wg_cdot(r0, v, n, tid, nthr, scr));
    T *sz = PC ? z : r;
    T w;
    // the second half of a step: r -= alpha v ; t = A s ; w ; x -= alpha y + w s ; r -= w t
    auto half = [&]() {
        const T na = sneg(alpha);
        BATCH_EACH(i) r[i] = sadd(r[i], smul(v[i], na));
        if (PC) { BATCH_EACH(i) z[i] = smul(r[i], dinv(i)); }
        wg_spmv(M, sz, t, n, tid, nthr);
        T tt = szero<T>(), tr = szero<T>();
        BATCH_EACH(i) { tt = sadd(tt, smul(sconj(t[i]), t[i])); tr = sadd(tr, smul(sconj(t[i]), r[i])); }
        wg_sum2(tt, tr, scr, tt, tr);
        w = sre(tt) > R(0) ? sdiv(tr, tt) : szero<T>();
        const T nw = sneg(w);
        BATCH_EACH(i) {
            x[i] = sadd(x[i], smul(y[i], na));
            x[i] = sadd(x[i], smul(sz[i], nw));
            r[i] = sadd(r[i], smul(t[i], nw));
        }
    };
    half();
    for (unsigned long long its = 1; its < a.max_iter; ++its) {
        R rs = 0;
        T rr = szero<T>();
        BATCH_EACH(i) { rs = rs + ssq(r[i]); rr = sadd(rr, smul(sconj(r0[i]), r[i])); }
        wg_sum2(rs, rr, scr, rs, rr);
        const R r_norm = ssqrt(rs);
        if (r_norm <= tol2) { batch_finish(a, b, x, xg, n, tid, nthr, SPRS_OK, its, r_norm / rhs_norm); return; }
        const T rho_old = rho;
        rho = rr;
        if (sabs(rho) < r0_norm_tol) {                       // restart
            wg_spmv(M, x, r, n, tid, nthr);
            BATCH_EACH(i) { r[i] = sadd(r[i], smul(rhs[i], mone)); r0[i] = r[i]; }
            const R rn = wg_norm2(r, n, tid, nthr, scr);
            rho = sfromr<T>(rn * rn);
            r0_norm_tol = sre(rho) * eps * eps;
        }
        const T beta = smul(sdiv(rho, rho_old), sdiv(alpha, w));
        const T c1 = smul(sneg(beta), w);
        T *yp = PC ? p : y;
        BATCH_EACH(i) {
            yp[i] = sadd(smul(v[i], c1), smul(yp[i], beta));
            yp[i] = sadd(yp[i], smul(r[i], one));
        }
        if (PC) { BATCH_EACH(i) y[i] = smul(p[i], dinv(i)); }
        wg_spmv(M, y, v, n, tid, nthr);
        const T tmp = wg_cdot(r0, v, n, tid, nthr, scr);
        if (sabs(tmp) <= R(0)) { batch_finish(a, b, x, xg, n, tid, nthr, SPRS_BREAKDOWN, its, R(0)); return; }
        alpha = sdiv(rho, tmp);
        half();
    }
    batch_finish(a, b, x, xg, n, tid, nthr, SPRS_INSUFFICIENT_ITER, a.max_iter, R(0));
}

// CG per system: the recurrence of sprs_cg_* in the header, with dinv_i = one / a_ii for the preconditioner (PC).
template <class T, bool PC>
__global__ __launch_bounds__(BLOCK) void batch_cg_kernel(BatchSolveArgs<T> a) {
    using R = Real<T>;
    const int n = a.D.n, tid = (int)threadIdx.x, nthr = (int)blockDim.x;
    const int64_t b = blockIdx.x;
    const SellDev<T> M = a.D.system(b);
    extern __shared__ __align__(16) unsigned char batch_lds[];   // all of it dynamic: the carve offsets stay multiples of 16
    unsigned char *scr = batch_lds;
    T *vec = reinterpret_cast<T *>(batch_lds + BATCH_SCRATCH);
    T *x = vec, *r = vec + n, *zz = vec + 2 * (size_t)n, *p = vec + 3 * (size_t)n, *q = vec + 4 * (size_t)n;
    T *z = PC ? zz : r;
    const T *rhs = a.rhs + b * n;
    T *xg = a.x + b * n;
    const R eps = seps<R>();
    const T one = sone<T>(), mone = sneg(sone<T>());
    auto dinv = [&](int i) { return sdiv(one, M.val[a.D.dslot[i]]); };

    const R rhs_norm = wg_norm2(rhs, n, tid, nthr, scr);
    if (rhs_norm <= eps) {
        BATCH_EACH(i) xg[i] = szero<T>();
        if (tid == 0) { a.its[b] = 0; a.res[b] = rhs_norm; a.status[b] = SPRS_OK; }
        return;
    }
    const R tol2 = a.tol * rhs_norm;
    BATCH_EACH(i) x[i] = xg[i];
    wg_spmv(M, x, r, n, tid, nthr);
    BATCH_EACH(i) r[i] = sadd(smul(rhs[i], one), smul(r[i], mone));
    R r_norm = wg_norm2(r, n, tid, nthr, scr);
    if (r_norm <= tol2) { batch_finish(a, b, x, xg, n, tid, nthr, SPRS_OK, 0, r_norm / rhs_norm); return; }
    if (PC) { BATCH_EACH(i) z[i] = smul(r[i], dinv(i)); }
    BATCH_EACH(i) p[i] = z[i];
    T rho = wg_cdot(r, z, n, tid, nthr, scr);
    for (unsigned long long its = 0; its < a.max_iter; ++its) {
        wg_spmv(M, p, q, n, tid, nthr);
        const T pq = wg_cdot(p, q, n, tid, nthr, scr);
        if (!(sre(pq) > R(0))) { batch_finish(a, b, x, xg, n, tid, nthr, SPRS_BREAKDOWN, its, R(0)); return; }
        const T alpha = sdiv(rho, pq), na = sneg(alpha);
        R rs = 0;
        T rz = szero<T>();
        BATCH_EACH(i) {
            x[i] = sadd(x[i], smul(p[i], alpha));
            r[i] = sadd(r[i], smul(q[i], na));
            if (PC) z[i] = smul(r[i], dinv(i));
            rs = rs + ssq(r[i]);
            rz = sadd(rz, smul(sconj(r[i]), z[i]));
        }
        wg_sum2(rs, rz, scr, rs, rz);
        r_norm = ssqrt(rs);
        if (r_norm <= tol2) { batch_finish(a, b, x, xg, n, tid, nthr, SPRS_OK, its + 1, r_norm / rhs_norm); return; }
        if (PC && !(sre(rz) > R(0))) { batch_finish(a, b, x, xg, n, tid, nthr, SPRS_INVALID_PRECOND, its, sre(rz)); return; }
        const T beta = sdiv(rz, rho);
        rho = rz;
        BATCH_EACH(i) p[i] = sadd(smul(z[i], one), smul(p[i], beta));
    }
    batch_finish(a, b, x, xg, n, tid, nthr, SPRS_INSUFFICIENT_ITER, a.max_iter, R(0));
}

// ---- host side
int scatter_grid(const sprs_ctx *c, int64_t total) { return balanced_grid(c, (total + BLOCK - 1) / BLOCK); }

template <class T>
BatchDev<T> batch_dev(const sprs_batch *B) {
    return BatchDev<T>{B->len, B->sbase, B->col, (const T *)B->val, B->dslot, B->slots, (int)B->n};
}

// the (nbatch, nnz) block `values` (device) into the packed layout; asynchronous on the context's stream
template <class T>
int batch_pack_values(sprs_batch *B, const T *values_dev) {
    sprs_ctx *c = B->ctx;
    const int64_t total = B->nbatch * B->nnz;
    if (!total) return SPRS_OK;
    hipLaunchKernelGGL(batch_scatter_kernel<T>, dim3(scatter_grid(c, total)), dim3(BLOCK), 0, c->stream, total, B->nnz, B->slots, B->dst, values_dev,
                       (T *)B->val);
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

template <class T>
int batch_set_values(sprs_batch *B, const T *values, bool host) {
    if (!B || B->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    const int64_t total = B->nbatch * B->nnz;
    if (!total) return SPRS_OK;
    if (!values) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = B->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    if (!host) {
        SPRS_TRY(batch_pack_values<T>(B, values));
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        return SPRS_OK;
    }
    DevBufs tmp;
    T *d;
    SPRS_TRY(tmp.alloc(c, &d, (size_t)total));
    SPRS_HIP_TRY(c, hipMemcpyAsync(d, values, sizeof(T) * (size_t)total, hipMemcpyHostToDevice, c->stream));
    SPRS_TRY(batch_pack_values<T>(B, d));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

template <class T>
int batch_read(const sprs_batch *B, T *values_host) {
    if (!B || B->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    const int64_t total = B->nbatch * B->nnz;
    if (!total) return SPRS_OK;
    if (!values_host) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = B->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    DevBufs tmp;
    T *d;
    SPRS_TRY(tmp.alloc(c, &d, (size_t)total));
    hipLaunchKernelGGL(batch_gather_kernel<T>, dim3(scatter_grid(c, total)), dim3(BLOCK), 0, c->stream, total, B->nnz, B->slots, B->dst, (const T *)B->val, d);
    SPRS_HIP_TRY(c, hipGetLastError());
    SPRS_HIP_TRY(c, hipMemcpyAsync(values_host, d, sizeof(T) * (size_t)total, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

// The pattern checked, packed and uploaded, the values packed.  rp / ci / values: host arrays (host) or device arrays.
template <class T>
int batch_create(sprs_ctx *c, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *rp_in, const int32_t *ci_in, const T *values, bool host,
                 sprs_batch **out, int64_t *row_out) {
    if (!out) return SPRS_INVALID_ARGUMENT;
    *out = nullptr;
    if (row_out) *row_out = -1;
    if (!c) return SPRS_INVALID_ARGUMENT;
    if (n < 0 || nnz < 0 || nbatch < 0) return refuse(c, "sprs_batch_create", "n = %lld, nnz = %lld and nbatch = %lld must not be negative", (long long)n, (long long)nnz, (long long)nbatch);
    if (!rp_in || (nnz && !ci_in)) return refuse(c, "sprs_batch_create", "the pattern is NULL");
    if (n > INT32_MAX - 64 || nnz > INT32_MAX) return refuse(c, "sprs_batch_create", "n = %lld or nnz = %lld is out of the int32 range", (long long)n, (long long)nnz);
    if (nbatch > INT32_MAX) return refuse(c, "sprs_batch_create", "nbatch = %lld is out of the int32 range", (long long)nbatch);
    if (nbatch && nnz && !values) return refuse(c, "sprs_batch_create", "values is NULL");
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    std::vector<int32_t> rp((size_t)n + 1), ci((size_t)nnz);
    if (host) {
        std::copy(rp_in, rp_in + n + 1, rp.begin());
        std::copy(ci_in, ci_in + nnz, ci.begin());
    } else {
        SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
        SPRS_HIP_TRY(c, hipMemcpy(rp.data(), rp_in, sizeof(int32_t) * rp.size(), hipMemcpyDeviceToHost));
        if (nnz) SPRS_HIP_TRY(c, hipMemcpy(ci.data(), ci_in, sizeof(int32_t) * ci.size(), hipMemcpyDeviceToHost));
    }
    if (rp[0] != 0 || rp[(size_t)n] != nnz) return refuse(c, "sprs_batch_create", "row_ptr must run from 0 to nnz = %lld", (long long)nnz);
    for (int64_t i = 0; i < n; ++i)
        if (rp[(size_t)i + 1] < rp[(size_t)i]) return refuse(c, "sprs_batch_create", "row_ptr decreases at row %lld", (long long)i);
    for (int64_t k = 0; k < nnz; ++k)
        if (ci[(size_t)k] < 0 || ci[(size_t)k] >= n) return refuse(c, "sprs_batch_create", "column index %d of entry %lld is outside [0, %lld)", ci[(size_t)k], (long long)k, (long long)n);
    for (int64_t i = 0; i < n; ++i)
        for (int32_t k = rp[(size_t)i] + 1; k < rp[(size_t)i + 1]; ++k)
            if (ci[(size_t)k] <= ci[(size_t)k - 1]) {
                if (row_out) *row_out = i;
                return refuse(c, "sprs_batch_create", "the column indices of row %lld are not strictly ascending", (long long)i);
            }
    auto *B = new sprs_batch();
    B->ctx = c; B->dtype = dtype_of<T>::value; B->n = n; B->nnz = nnz; B->nbatch = nbatch;
    auto fail = [&](int st) { sprs_batch_destroy(B); return st; };
    // the layout, packed with the entries' own numbers for values: slot -> CSR entry + 1 (0: padding)
    std::vector<int32_t> number((size_t)nnz);
    std::iota(number.begin(), number.end(), 1);
    const SellPacked<int32_t> S = sell_pack<int32_t>(
        n, [](size_t p) { return (int32_t)p; }, [&](int32_t i) { return rp[(size_t)i]; }, [&](int32_t i) { return rp[(size_t)i + 1]; }, ci.data(),
        number.data());
    if (S.slots > INT32_MAX) return fail(refuse(c, "sprs_batch_create", "the packed layout has more than 2^31 - 1 slots"));
    B->slots = S.slots;
    std::vector<int32_t> dst((size_t)nnz), dslot((size_t)n, -1);
    for (int64_t s = 0; s < S.slots; ++s)
        if (S.val[(size_t)s]) dst[(size_t)S.val[(size_t)s] - 1] = (int32_t)s;
    for (int64_t i = n - 1; i >= 0; --i) {
        const int64_t d = diag_pos(rp.data(), ci.data(), i);
        if (d < 0) B->nodiag_row = i;
        else dslot[(size_t)i] = dst[(size_t)d];
    }
    if (!dev_upload(&B->len, S.len.data(), S.len.size()) || !dev_upload(&B->sbase, S.sbase.data(), S.sbase.size()) ||
        !dev_upload(&B->col, S.col.data(), S.col.size()) || !dev_upload(&B->dst, dst.data(), dst.size()) ||
        !dev_upload(&B->dslot, dslot.data(), dslot.size()))
        return fail(SPRS_ERR_HIP);
    const size_t nval = (size_t)nbatch * (size_t)S.slots, nb = (size_t)nbatch;
    if (hipMalloc(&B->val, sizeof(T) * (nval + 2)) != hipSuccess || hipMalloc((void **)&B->d_its, sizeof(unsigned long long) * (nb + 1)) != hipSuccess ||
        hipMalloc(&B->d_res, sizeof(Real<T>) * (nb + 1)) != hipSuccess || hipMalloc((void **)&B->d_status, sizeof(int) * (nb + 1)) != hipSuccess)
        return fail(SPRS_ERR_HIP);
    if (hipMemsetAsync(B->val, 0, sizeof(T) * (nval + 2), c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return fail(SPRS_ERR_HIP);
    const int st = batch_set_values<T>(B, values, host);
    if (st != SPRS_OK) return fail(st);
    *out = B;
    return SPRS_OK;
}

// the two staging blocks of the host entry points
template <class T>
int batch_staging(sprs_batch *B) {
    sprs_ctx *c = B->ctx;
    const size_t total = (size_t)B->nbatch * (size_t)B->n;
    if (!B->a_tmp) SPRS_HIP_TRY(c, hipMalloc(&B->a_tmp, sizeof(T) * (total + 2)));
    if (!B->b_tmp) SPRS_HIP_TRY(c, hipMalloc(&B->b_tmp, sizeof(T) * (total + 2)));
    return SPRS_OK;
}

template <class T>
int batch_mul_vec(const sprs_batch *Bc, const T *x, size_t xl, T *y, size_t yl, bool host) {
    if (!Bc || Bc->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    sprs_batch *B = const_cast<sprs_batch *>(Bc);
    const size_t total = (size_t)B->nbatch * (size_t)B->n;
    if (xl != total || yl != total) return SPRS_DIM_MISMATCH;
    if (!total) return SPRS_OK;
    if (!x || !y) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = B->ctx;
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    const T *dx = x;
    T *dy = y;
    if (host) {
        SPRS_TRY(batch_staging<T>(B));
        SPRS_HIP_TRY(c, hipMemcpyAsync(B->a_tmp, x, sizeof(T) * total, hipMemcpyHostToDevice, c->stream));
        dx = (const T *)B->a_tmp; dy = (T *)B->b_tmp;
    }
    hipLaunchKernelGGL(batch_mul_vec_kernel<T>, dim3((unsigned)B->nbatch), dim3(batch_threads(B->n)), 0, c->stream, batch_dev<T>(B), dx, dy);
    SPRS_HIP_TRY(c, hipGetLastError());
    if (host) SPRS_HIP_TRY(c, hipMemcpyAsync(y, dy, sizeof(T) * total, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SPRS_OK;
}

template <class T, class K>
int batch_launch(sprs_ctx *c, K kernel, const BatchSolveArgs<T> &a, int64_t nbatch, size_t lds) {
    if (lds > ((size_t)64 << 10)) SPRS_HIP_TRY(c, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)nbatch), dim3(batch_threads(a.D.n)), lds, c->stream, a);
    SPRS_HIP_TRY(c, hipGetLastError());
    return SPRS_OK;
}

template <class T>
int batch_solve(sprs_batch *B, int solver, bool host, int precond, const T *rhs, size_t rl, T *x, size_t xl, size_t max_iter, Real<T> tol, size_t *its_out,
                Real<T> *res_out, int *status_out) {
    using R = Real<T>;
    if (!B || B->dtype != dtype_of<T>::value) return SPRS_INVALID_ARGUMENT;
    sprs_ctx *c = B->ctx;
    const char *who = solver == BATCH_CG ? "sprs_batch_cg_solve" : "sprs_batch_bicgstab_solve";
    if (precond != SPRS_BATCH_NONE && precond != SPRS_BATCH_JACOBI)
        return refuse(c, who, "precond must be SPRS_BATCH_NONE or SPRS_BATCH_JACOBI (got %d)", precond);
    const size_t total = (size_t)B->nbatch * (size_t)B->n;
    if (rl != total) return SPRS_INCOMPATIBLE_RHS_SIZE;
    if (xl != total) return SPRS_INCOMPATIBLE_X_SIZE;
    if (!total) return SPRS_OK;
    if (!rhs || !x) return SPRS_INVALID_ARGUMENT;
    const int64_t cap = batch_max_rows(solver, (int64_t)sizeof(T));
    if (B->n > cap)
        return refuse(c, who, "n = %lld is above this solver's cap of %lld rows for this scalar type (every vector of a system lives in one workgroup's LDS)",
                      (long long)B->n, (long long)cap);
    if (precond == SPRS_BATCH_JACOBI && B->nodiag_row >= 0) {
        snprintf(c->err, sizeof(c->err), "%s: row %lld stores no diagonal entry (Jacobi needs every one)", who, (long long)B->nodiag_row);
        if (its_out) its_out[0] = (size_t)B->nodiag_row;
        return SPRS_ZERO_DIAGONAL;
    }
    CtxLock lock(c);
    SPRS_HIP_TRY(c, hipSetDevice(c->device));
    const T *drhs = rhs;
    T *dx = x;
    if (host) {
        SPRS_TRY(batch_staging<T>(B));
        SPRS_HIP_TRY(c, hipMemcpyAsync(B->a_tmp, rhs, sizeof(T) * total, hipMemcpyHostToDevice, c->stream));
        SPRS_HIP_TRY(c, hipMemcpyAsync(B->b_tmp, x, sizeof(T) * total, hipMemcpyHostToDevice, c->stream));
        drhs = (const T *)B->a_tmp; dx = (T *)B->b_tmp;
    }
    const BatchSolveArgs<T> a{batch_dev<T>(B), drhs, dx, (unsigned long long)max_iter, tol, B->d_its, (R *)B->d_res, B->d_status};
    const size_t lds = (size_t)batch_lds_bytes(solver, (int64_t)sizeof(T), B->n);
    const bool pc = precond == SPRS_BATCH_JACOBI;
    if (solver == BATCH_CG) SPRS_TRY(pc ? batch_launch<T>(c, batch_cg_kernel<T, true>, a, B->nbatch, lds) : batch_launch<T>(c, batch_cg_kernel<T, false>, a, B->nbatch, lds));
    else SPRS_TRY(pc ? batch_launch<T>(c, batch_bicgstab_kernel<T, true>, a, B->nbatch, lds) : batch_launch<T>(c, batch_bicgstab_kernel<T, false>, a, B->nbatch, lds));
    const size_t nb = (size_t)B->nbatch;
    std::vector<unsigned long long> its(nb);
    std::vector<R> res(nb);
    std::vector<int> status(nb);
    if (host) SPRS_HIP_TRY(c, hipMemcpyAsync(x, dx, sizeof(T) * total, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipMemcpyAsync(its.data(), B->d_its, sizeof(unsigned long long) * nb, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipMemcpyAsync(res.data(), B->d_res, sizeof(R) * nb, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipMemcpyAsync(status.data(), B->d_status, sizeof(int) * nb, hipMemcpyDeviceToHost, c->stream));
    SPRS_HIP_TRY(c, hipStreamSynchronize(c->stream));
    int ret = SPRS_OK;
    for (size_t j = 0; j < nb; ++j) {
        if (its_out) its_out[j] = (size_t)its[j];
        if (res_out) res_out[j] = res[j];
        if (status_out) status_out[j] = status[j];
        if (ret == SPRS_OK && status[j] != SPRS_OK) ret = status[j];
    }
    return ret;
}

}  // namespace

#define SPRS_G(...) try { __VA_ARGS__ } catch (...) { return SPRS_ERR_HIP; }

extern "C" {

int sprs_batch_destroy(sprs_batch *B) {
    if (!B) return SPRS_OK;
    if (B->ctx) { (void)hipSetDevice(B->ctx->device); (void)hipStreamSynchronize(B->ctx->stream); }
    for (void *p : {(void *)B->len, (void *)B->col, (void *)B->sbase, (void *)B->dst, (void *)B->dslot, B->val, (void *)B->d_its, B->d_res,
                    (void *)B->d_status, B->a_tmp, B->b_tmp})
        if (p) (void)hipFree(p);
    delete B;
    return SPRS_OK;
}

int sprs_batch_info(const sprs_batch *B, int64_t *n, int64_t *nnz, int64_t *nbatch, int64_t *threads, int64_t *lds_cg, int64_t *lds_bicgstab) {
    if (!B) return SPRS_INVALID_ARGUMENT;
    const int64_t sz = batch_scalar_bytes(B->dtype);
    if (n) *n = B->n;
    if (nnz) *nnz = B->nnz;
    if (nbatch) *nbatch = B->nbatch;
    if (threads) *threads = batch_threads(B->n);
    if (lds_cg) *lds_cg = batch_lds_bytes(BATCH_CG, sz, B->n);
    if (lds_bicgstab) *lds_bicgstab = batch_lds_bytes(BATCH_BICGSTAB, sz, B->n);
    return SPRS_OK;
}

int sprs_batch_max_rows(int solver, int dtype) { return (int)batch_max_rows(solver, batch_scalar_bytes(dtype)); }

#define SPRS_BATCH_API(X, T, CT, R)                                                                                                                   \
    int sprs_batch_create_##X(sprs_ctx *ctx, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *rp, const int32_t *ci, const CT *v, sprs_batch **out, \
                              int64_t *row_out) {                                                                                                     \
        SPRS_G(return batch_create<T>(ctx, n, nnz, nbatch, rp, ci, (const T *)v, true, out, row_out);)                                                \
    }                                                                                                                                                 \
    int sprs_batch_create_dev_##X(sprs_ctx *ctx, int64_t n, int64_t nnz, int64_t nbatch, const int32_t *rp, const int32_t *ci, const CT *v,          \
                                  sprs_batch **out, int64_t *row_out) {                                                                               \
        SPRS_G(return batch_create<T>(ctx, n, nnz, nbatch, rp, ci, (const T *)v, false, out, row_out);)                                               \
    }                                                                                                                                                 \
    int sprs_batch_set_values_##X(sprs_batch *B, const CT *v) { SPRS_G(return batch_set_values<T>(B, (const T *)v, true);) }                          \
    int sprs_batch_set_values_dev_##X(sprs_batch *B, const CT *v) { SPRS_G(return batch_set_values<T>(B, (const T *)v, false);) }                     \
    int sprs_batch_read_##X(const sprs_batch *B, CT *v) { SPRS_G(return batch_read<T>(B, (T *)v);) }                                                  \
    int sprs_batch_mul_vec_##X(const sprs_batch *B, const CT *x, size_t xl, CT *y, size_t yl) {                                                       \
        SPRS_G(return batch_mul_vec<T>(B, (const T *)x, xl, (T *)y, yl, true);)                                                                       \
    }                                                                                                                                                 \
    int sprs_batch_mul_vec_dev_##X(const sprs_batch *B, const CT *x, size_t xl, CT *y, size_t yl) {                                                   \
        SPRS_G(return batch_mul_vec<T>(B, (const T *)x, xl, (T *)y, yl, false);)                                                                      \
    }                                                                                                                                                 \
    int sprs_batch_bicgstab_solve_##X(sprs_batch *B, int pc, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res, int *status) { \
        SPRS_G(return batch_solve<T>(B, BATCH_BICGSTAB, true, pc, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res, status);)                        \
    }                                                                                                                                                 \
    int sprs_batch_bicgstab_solve_dev_##X(sprs_batch *B, int pc, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res, int *status) { \
        SPRS_G(return batch_solve<T>(B, BATCH_BICGSTAB, false, pc, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res, status);)                       \
    }                                                                                                                                                 \
    int sprs_batch_cg_solve_##X(sprs_batch *B, int pc, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res, int *status) { \
        SPRS_G(return batch_solve<T>(B, BATCH_CG, true, pc, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res, status);)                              \
    }                                                                                                                                                 \
    int sprs_batch_cg_solve_dev_##X(sprs_batch *B, int pc, const CT *rhs, size_t rl, CT *x, size_t xl, size_t mi, R tol, size_t *its, R *res, int *status) { \
        SPRS_G(return batch_solve<T>(B, BATCH_CG, false, pc, (const T *)rhs, rl, (T *)x, xl, mi, tol, its, res, status);)                             \
    }
SPRS_BATCH_API(d, double, double, double)
SPRS_BATCH_API(z, cplx, sprs_c64, double)
SPRS_BATCH_API(s, float, float, float)
SPRS_BATCH_API(c, cplxf, sprs_c32, float)

}  // extern "C"
