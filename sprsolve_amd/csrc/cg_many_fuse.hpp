// Batched conjugate gradients: the vector kernels of CgMany<T> (cg_many.hip), CgKB / CgKC (cg_fuse.hpp) for a block of k <= 8
// right-hand sides, run by fused_kernel (fused_launch.hpp) over the n_pad * KP elements of a block.  Every column runs the recurrence of the header's sprs_cg_* comment on its own scalars.  A fused
// iteration is three launches whatever k is:
//   SpMM      Q = A P with the per-column partials of conj(p_c).q_c                          (spmm.hip)
//   CgManyKB  alpha_c = rho_c / (p_c.q_c) ; x += p alpha ; r += q (-alpha) ; [z = M^-1 r] ; partials of |r_c|^2, conj(r_c).z_c
//   CgManyKC  r_norm_c, convergence ; rho_new_c, beta_c ; p = z 1 + p beta
// and a solve starts with CgManyS0 (partials of |rhs_c|^2), one SpMM (A x), CgManyS1 (zero right-hand sides, r, z, p and the
// partials of |r_c|^2, conj(r_c).z_c) and CgManyS2 (converged at the start?, rho_c, the count of running columns).
//
// Layout: the work vectors are row-major blocks with a column stride KP = the next power of two >= the handle's k, and
// their row count is padded to a multiple of 4, so that a block is a whole number of 16-byte packs and a lane's pack covers
// the same columns on every trip of its grid-stride walk (the stride, a multiple of 256 packs, is a multiple of the KP / PK
// packs of a row): the lane keeps one accumulator per pack element.  Padding columns carry a zero right-hand side and
// padding rows are skipped, so neither is ever touched.
//
// State rules (CgManyState):
//   * status[c] leaves ST_RUNNING once; from then on column c is frozen: no kernel changes its x, r or p (a pack that also
//     holds running columns is stored with the frozen column's elements as they were loaded).  The kernels BRANCH on the
//     column's status — a multiplication by alpha = 0 would let a NaN column leak into nothing but would rewrite it.
//   * `running` counts the columns whose status is ST_RUNNING; once it is zero every later launch, the SpMM included,
//     returns at its first instruction.
//   * A launch reads only fields that none of its workgroups writes (rho_prev[c] is rho[c] as KB read it), with the
//     exception CgKB makes too: status[c] and `running` are written by workgroup 0 from values every workgroup computes for
//     itself, so a reader that sees the new value takes the branch it would have taken anyway.
#pragma once
#include "fused_launch.hpp"

namespace sprs {

constexpr int CGM_MAXK = 8;
// column states beside ST_RUNNING / ST_CONVERGED / ST_BREAKDOWN / ST_INVALID_PC
enum : int { CGM_ZERO_RHS = 16, CGM_UNUSED = 17 };

template <class T>
struct CgManyState {
    T rho[CGM_MAXK], rho_prev[CGM_MAXK], alpha[CGM_MAXK], beta[CGM_MAXK];
    Real<T> r_norm[CGM_MAXK], tol2[CGM_MAXK], pc_re[CGM_MAXK], rhs_norm[CGM_MAXK];
    long long its[CGM_MAXK];     // completed iterations of the column = the 0-based index of its running one
    int status[CGM_MAXK];
    int running, pad[3];
};

// a[c] for a lane-dependent c without indexing registers dynamically (complex values component by component: a select
// between two structs becomes a select between their addresses, i.e. an array in scratch memory)
__device__ __forceinline__ double cgm_sel(bool t, double a, double b) { return t ? a : b; }
__device__ __forceinline__ float cgm_sel(bool t, float a, float b) { return t ? a : b; }
__device__ __forceinline__ bool cgm_sel(bool t, bool a, bool b) { return t ? a : b; }
__device__ __forceinline__ cplx cgm_sel(bool t, cplx a, cplx b) { return cplx{t ? a.re : b.re, t ? a.im : b.im}; }
__device__ __forceinline__ cplxf cgm_sel(bool t, cplxf a, cplxf b) { return cplxf{t ? a.re : b.re, t ? a.im : b.im}; }
template <class U>
__device__ __forceinline__ U cgm_pick(const U (&a)[CGM_MAXK], int c) {
    U r = a[0];
#pragma unroll
    for (int j = 1; j < CGM_MAXK; ++j) r = cgm_sel(c == j, a[j], r);
    return r;
}

// Sums over the workgroup of the first kp of 8 per-thread values; block_sum's order (butterfly, then waves left to right)
// per value, one pair of barriers for all of them.  sm: CGM_MAXK * NWAVE elements.
template <class U>
__device__ __forceinline__ void cgm_block_sums(U (&v)[CGM_MAXK], int kp, U *sm) {
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < CGM_MAXK; ++c)
        if (c < kp) v[c] = wave_sum(v[c]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c)
            if (c < kp) sm[c * NWAVE + wv] = v[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < CGM_MAXK; ++c) {
        if (c < kp) {
            U a = sm[c * NWAVE];
#pragma unroll
            for (int w = 1; w < NWAVE; ++w) a = sadd(a, sm[c * NWAVE + w]);
            v[c] = a;
        }
    }
}

// The consumer's prologue: every workgroup re-reduces the kp rows [column][workgroup] of one or two partial arrays in the
// same fixed order (thread t adds partials t, t + 256, ..; then cgm_block_sums) => the same bits in every workgroup.  The
// loads of all columns of both arrays of a trip are issued before any is consumed.
template <class UA, class UB, bool TWO>
__device__ __forceinline__ void cgm_reduce(const UA *__restrict__ pa, const UB *__restrict__ pb, int stride, int P, int kp,
                                           UA (&ra)[CGM_MAXK], UB (&rb)[CGM_MAXK], UA *smA, UB *smB) {
#pragma unroll
    for (int c = 0; c < CGM_MAXK; ++c) { ra[c] = szero<UA>(); rb[c] = szero<UB>(); }
    for (int i = threadIdx.x; i < P; i += BLOCK) {
        UA va[CGM_MAXK]; UB vb[CGM_MAXK];
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c) {
            if (c < kp) {
                va[c] = pa[(size_t)c * stride + i];
                if (TWO) vb[c] = pb[(size_t)c * stride + i];
            }
        }
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c) {
            if (c < kp) {
                ra[c] = sadd(ra[c], va[c]);
                if (TWO) rb[c] = sadd(rb[c], vb[c]);
            }
        }
    }
    cgm_block_sums(ra, kp, smA);
    if (TWO) cgm_block_sums(rb, kp, smB);
}

// What the functors share: the lane's columns, its per-element accumulators and their hand-over as partials.
template <class T>
struct CgManyLane {
    static constexpr int PKW = pack_width<T>::value;
    int col[PKW];                // column of pack element e (the same on every trip)
    bool act[PKW];               // ... and whether that column is updated by this launch
    Real<T> accN[PKW]; T accR[PKW];
    __device__ __forceinline__ void init(int kp) {
#pragma unroll
        for (int e = 0; e < PKW; ++e) {
            col[e] = (int)((threadIdx.x * PKW + e) & (unsigned)(kp - 1));
            act[e] = false; accN[e] = 0.0; accR[e] = szero<T>();
        }
    }
    // row of element e of pack i (lg = log2 of the column stride)
    template <int PK> __device__ __forceinline__ static int64_t row_of(int64_t i, int e, int lg) { return (i * PK + e) >> lg; }
    // partials of this workgroup: [column][workgroup]
    template <bool TWO> __device__ __forceinline__ void hand_over(int kp, Real<T> *partN, T *partRZ) {
        __shared__ Real<T> smD[CGM_MAXK * NWAVE];
        __shared__ T smT[CGM_MAXK * NWAVE];
        Real<T> a[CGM_MAXK]; T b[CGM_MAXK];
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c) {
            a[c] = 0.0; b[c] = szero<T>();
#pragma unroll
            for (int e = 0; e < PKW; ++e) {
                if (col[e] == c) { a[c] = a[c] + accN[e]; if (TWO) b[c] = sadd(b[c], accR[e]); }
            }
        }
        cgm_block_sums(a, kp, smD);
        if (TWO) cgm_block_sums(b, kp, smT);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < CGM_MAXK; ++c) {
                if (c < kp) {
                    partN[(size_t)c * gridDim.x + blockIdx.x] = a[c];
                    if (TWO) partRZ[(size_t)c * gridDim.x + blockIdx.x] = b[c];
                }
            }
        }
    }
};

// S0: partials of |rhs_c|^2 (rhs sits in r)
template <class T>
struct CgManyS0 {
    const T *r; Real<T> *partN; int kp, lg; int64_t n;
    CgManyLane<T> L;
    static constexpr bool whole_packs = true;      // a block is whole packs: fused_kernel (fused_launch.hpp) needs no scalar tail
    __device__ __forceinline__ bool prologue() { L.init(kp); return true; }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        const auto rv = ldp<T, PK, NT>(r, i);
#pragma unroll
        for (int e = 0; e < PK; ++e)
            if (L.template row_of<PK>(i, e, lg) < n) L.accN[e] = L.accN[e] + ssq(rv.v[e]);
    }
    __device__ __forceinline__ void epilogue() { L.template hand_over<false>(kp, partN, nullptr); }
};

// S1: rhs_norm_c ; zero right-hand side (x_c = 0, done) ; tol2_c = tol rhs_norm_c ; r = rhs*1 + (A x)*(-1) ; z = M^-1 r ;
//     p = z ; partials of |r_c|^2 and conj(r_c).z_c.  rhs sits in r, A x in q.
template <class T, class V, bool PC>
struct CgManyS1 {
    CgManyState<T> *S; const Real<T> *partRhs; int P; Real<T> tol;
    const T *q; T *x; T *r; T *p; const V *dinv; T *z; Real<T> *partN; T *partRZ; int kp, lg; int64_t n;
    CgManyLane<T> L;
    bool zero[CgManyLane<T>::PKW];
    static constexpr bool whole_packs = true;
    __device__ __forceinline__ bool prologue() {
        __shared__ Real<T> smD[CGM_MAXK * NWAVE];
        Real<T> sN[CGM_MAXK], dummy[CGM_MAXK];
        cgm_reduce<Real<T>, Real<T>, false>(partRhs, partRhs, P, P, kp, sN, dummy, smD, smD);
        L.init(kp);
        bool zc[CGM_MAXK];
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c) {
            zc[c] = false;
            if (c < kp) {
                const Real<T> rhs_norm = ssqrt(sN[c]);
                zc[c] = rhs_norm <= seps<Real<T>>();                 // bicg_stab.rs:56-60 (a NaN norm is not zero)
                if (first_thread()) { S->rhs_norm[c] = rhs_norm; S->tol2[c] = tol * rhs_norm; S->status[c] = zc[c] ? (int)CGM_ZERO_RHS : (int)ST_RUNNING; }
            }
        }
#pragma unroll
        for (int e = 0; e < CgManyLane<T>::PKW; ++e) { zero[e] = cgm_pick(zc, L.col[e]); L.act[e] = !zero[e]; }
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto rv = ldp<T, PK, NT>(r, i); const auto qv = ldp<T, PK, NT>(q, i);
        Pack<T, PK> zv = rv, xv;
        bool any_zero = false;
#pragma unroll
        for (int e = 0; e < PK; ++e) any_zero = any_zero || zero[e];
        if (any_zero) xv = ldp<T, PK, NT>(x, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            const int64_t row = L.template row_of<PK>(i, e, lg);
            if (row >= n) continue;
            if (zero[e]) { xv.v[e] = szero<T>(); continue; }
            const T rr = sadd(smul(rv.v[e], sone<T>()), smul(qv.v[e], sneg(sone<T>())));   // r = rhs*1 + (A x)*(-1)
            rv.v[e] = rr;
            T zz = rr;
            if (PC) { zz = smulv(rr, dinv[row]); }
            zv.v[e] = zz;
            L.accN[e] = L.accN[e] + ssq(rr);
            L.accR[e] = sadd(L.accR[e], smul(sconj(rr), zz));
        }
        stp<T, PK, NT>(r, i, rv);
        stp<T, PK, NT>(p, i, zv);                                     // p = z (a zero column's p holds its rhs: never read)
        if (PC) stp<T, PK, NT>(z, i, zv);
        if (any_zero) stp<T, PK, NT>(x, i, xv);
    }
    __device__ __forceinline__ void epilogue() { L.template hand_over<true>(kp, partN, partRZ); }
};

// S2 (one workgroup, no vector work): converged at the start? ; rho_c = conj(r_c).z_c ; running = the columns that iterate
template <class T>
struct CgManyS2 {
    CgManyState<T> *S; const Real<T> *partN; const T *partRZ; int P; int kp;
    static constexpr bool whole_packs = true;
    __device__ __forceinline__ bool prologue() {
        __shared__ Real<T> smD[CGM_MAXK * NWAVE];
        __shared__ T smT[CGM_MAXK * NWAVE];
        int status[CGM_MAXK]; Real<T> tol2[CGM_MAXK];
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c)
            if (c < kp) { status[c] = S->status[c]; tol2[c] = S->tol2[c]; }
        Real<T> sN[CGM_MAXK]; T sR[CGM_MAXK];
        cgm_reduce<Real<T>, T, true>(partN, partRZ, P, P, kp, sN, sR, smD, smT);
        int running = 0;
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c) {
            if (c < kp && status[c] == ST_RUNNING) {
                const Real<T> r_norm = ssqrt(sN[c]);
                if (r_norm <= tol2[c]) {
                    if (first_thread()) { S->r_norm[c] = r_norm; S->status[c] = ST_CONVERGED; }
                } else {
                    ++running;
                    if (first_thread()) { S->r_norm[c] = r_norm; S->rho[c] = sR[c]; S->rho_prev[c] = sR[c]; }
                }
            }
        }
        if (first_thread()) S->running = running;
        return false;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t) {}
    __device__ __forceinline__ void epilogue() {}
};

// KB (CgKB per column).  Reads x, p, r, q (+ dinv), writes x, r (+ z).
template <class T, class V, bool PC>
struct CgManyKB {
    CgManyState<T> *S; const T *partPQ; int strideQ; int P;
    const T *p; const T *q; T *x; T *r; const V *dinv; T *z; Real<T> *partN; T *partRZ; int kp, lg; int64_t n;
    CgManyLane<T> L;
    T alpha[CgManyLane<T>::PKW], na[CgManyLane<T>::PKW];
    static constexpr bool whole_packs = true;
    __device__ __forceinline__ bool prologue() {
        const int running = S->running;
        if (running == 0) return false;
        __shared__ T smT[CGM_MAXK * NWAVE];
        int status[CGM_MAXK]; T rho[CGM_MAXK];
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c) {
            status[c] = (int)CGM_UNUSED; rho[c] = szero<T>();
            if (c < kp) { status[c] = S->status[c]; rho[c] = S->rho[c]; }           // requested together with the partials
        }
        T pq[CGM_MAXK], dummy[CGM_MAXK];
        cgm_reduce<T, T, false>(partPQ, partPQ, strideQ, P, kp, pq, dummy, smT, smT);
        L.init(kp);
        // (every column's quotient is formed, used or not: branch-free values stay in registers)
        T al[CGM_MAXK]; bool on[CGM_MAXK];
        int stopped = 0, live = 0;
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c) {
            const bool runs = c < kp && status[c] == ST_RUNNING;
            const bool bad = !(sre(pq[c]) > 0.0);                               // not positive definite along p_c (a NaN lands here too)
            al[c] = sdiv(rho[c], pq[c]);
            on[c] = runs && !bad;
            stopped += runs && bad ? 1 : 0; live += on[c] ? 1 : 0;
            if (first_thread() && runs) {
                if (bad) S->status[c] = ST_BREAKDOWN;
                else { S->alpha[c] = al[c]; S->rho_prev[c] = rho[c]; }
            }
        }
        if (stopped && first_thread()) S->running = running - stopped;
        if (live == 0) return false;
#pragma unroll
        for (int e = 0; e < CgManyLane<T>::PKW; ++e) { L.act[e] = cgm_pick(on, L.col[e]); alpha[e] = cgm_pick(al, L.col[e]); na[e] = sneg(alpha[e]); }
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        bool any = false;
#pragma unroll
        for (int e = 0; e < PK; ++e) any = any || L.act[e];
        if (!any) return;                                                       // a pack of frozen columns is neither read nor written
        auto xv = ldp<T, PK, NT>(x, i); const auto pv = ldp<T, PK, NT>(p, i); auto rv = ldp<T, PK, NT>(r, i); const auto qv = ldp<T, PK, NT>(q, i);
        [[maybe_unused]] Pack<T, PK> zv;
        if (PC) zv = ldp<T, PK, NT>(z, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            const int64_t row = L.template row_of<PK>(i, e, lg);
            if (!L.act[e] || row >= n) continue;
            xv.v[e] = sadd(xv.v[e], smul(pv.v[e], alpha[e]));                   // axpy(alpha, p, x)
            const T rr = sadd(rv.v[e], smul(qv.v[e], na[e]));                   // axpy(-alpha, q, r)
            rv.v[e] = rr;
            T zz = rr;
            if (PC) { zz = smulv(rr, dinv[row]); zv.v[e] = zz; }                // z = M^-1 r
            L.accN[e] = L.accN[e] + ssq(rr);
            L.accR[e] = sadd(L.accR[e], smul(sconj(rr), zz));                   // conj_dot(r, z)
        }
        stp<T, PK, NT>(x, i, xv);
        stp<T, PK, NT>(r, i, rv);
        if (PC) stp<T, PK, NT>(z, i, zv);
    }
    __device__ __forceinline__ void epilogue() { L.template hand_over<true>(kp, partN, partRZ); }
};

// KC (CgKC per column).  Reads z (= r without a preconditioner) and p, writes p.
template <class T, bool PC>
struct CgManyKC {
    CgManyState<T> *S; const Real<T> *partN; const T *partRZ; int P;
    const T *z; T *p; int kp, lg; int64_t n;
    CgManyLane<T> L;
    T beta[CgManyLane<T>::PKW];
    static constexpr bool whole_packs = true;
    __device__ __forceinline__ bool prologue() {
        const int running = S->running;
        if (running == 0) return false;
        __shared__ Real<T> smD[CGM_MAXK * NWAVE];
        __shared__ T smT[CGM_MAXK * NWAVE];
        // only fields that no workgroup of THIS launch writes (rho, beta, r_norm, its are written below)
        int status[CGM_MAXK]; Real<T> tol2[CGM_MAXK]; T rho[CGM_MAXK];
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c) {
            status[c] = (int)CGM_UNUSED; tol2[c] = 0.0; rho[c] = szero<T>();
            if (c < kp) { status[c] = S->status[c]; tol2[c] = S->tol2[c]; rho[c] = S->rho_prev[c]; }
        }
        Real<T> sN[CGM_MAXK]; T sR[CGM_MAXK];
        cgm_reduce<Real<T>, T, true>(partN, partRZ, P, P, kp, sN, sR, smD, smT);
        L.init(kp);
        T be[CGM_MAXK]; bool on[CGM_MAXK];
        int stopped = 0, live = 0;
#pragma unroll
        for (int c = 0; c < CGM_MAXK; ++c) {
            const bool runs = c < kp && status[c] == ST_RUNNING;
            const Real<T> r_norm = ssqrt(sN[c]);
            const bool conv = r_norm <= tol2[c];
            const bool bad_pc = PC && !conv && !(sre(sR[c]) > 0.0);
            be[c] = sdiv(sR[c], rho[c]);
            on[c] = runs && !conv && !bad_pc;
            stopped += runs && !on[c] ? 1 : 0; live += on[c] ? 1 : 0;
            if (first_thread() && runs) {
                S->r_norm[c] = r_norm;
                if (conv) { S->its[c] = S->its[c] + 1; S->status[c] = ST_CONVERGED; }
                else if (bad_pc) { S->pc_re[c] = sre(sR[c]); S->status[c] = ST_INVALID_PC; }
                else { S->rho[c] = sR[c]; S->beta[c] = be[c]; S->its[c] = S->its[c] + 1; }
            }
        }
        if (stopped && first_thread()) S->running = running - stopped;
        if (live == 0) return false;
#pragma unroll
        for (int e = 0; e < CgManyLane<T>::PKW; ++e) { L.act[e] = cgm_pick(on, L.col[e]); beta[e] = cgm_pick(be, L.col[e]); }
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        bool any = false;
#pragma unroll
        for (int e = 0; e < PK; ++e) any = any || L.act[e];
        if (!any) return;
        const auto zv = ldp<T, PK, NT>(z, i); auto pv = ldp<T, PK, NT>(p, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            if (!L.act[e] || L.template row_of<PK>(i, e, lg) >= n) continue;
            pv.v[e] = sadd(smul(zv.v[e], sone<T>()), smul(pv.v[e], beta[e]));   // axpby(1, z, beta, p)
        }
        stp<T, PK, NT>(p, i, pv);
    }
    __device__ __forceinline__ void epilogue() {}
};

// rows x k (leading dimension k) <-> rows_pad x KP blocks; the padding of `dst` is zeroed by to_block
template <class T>
__global__ __launch_bounds__(BLOCK) void cg_many_to_block(int64_t n, int64_t n_pad, int k, int lg, const T *__restrict__ src, T *__restrict__ dst) {
    const int64_t tot = n_pad << lg;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < tot; i += (int64_t)gridDim.x * BLOCK) {
        const int64_t row = i >> lg; const int c = (int)(i & ((1 << lg) - 1));
        dst[i] = (row < n && c < k) ? src[row * k + c] : szero<T>();
    }
}
template <class T>
__global__ __launch_bounds__(BLOCK) void cg_many_from_block(int64_t n, int k, int lg, const T *__restrict__ src, T *__restrict__ dst) {
    const int64_t tot = n * k;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < tot; i += (int64_t)gridDim.x * BLOCK) {
        const int64_t row = i / k; const int c = (int)(i - row * k);
        dst[i] = src[(row << lg) + c];
    }
}

}  // namespace sprs
