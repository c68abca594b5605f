// BiCGStab's vector-update kernels (host: bicgstab.hip), K1 and K3 as structures other translation units can run: the plane-streaming
// chain SpMV (spmv_chain.hip) executes their PROLOGUES (the scalar logic of the recurrence: convergence / restart / breakdown
// tests, beta, alpha) at the top of its own launch and forms their element-wise results while it stages its x windows — the
// updated vector is consumed without a pass of its own ("fused SpMV input", bicgstab.hip).
#pragma once
#include "fused_launch.hpp"
#include "krylov.hpp"

namespace sprs {

// ======================================================================= BiCGStab kernels
// K1  bicg_stab.rs:123-156 (+ :321-328 with a preconditioner)
//   r_norm = norm2(r); converged?  rho = r0.r; restart?  beta = (rho/rho_old)*(alpha/w)
//   p = v*(-beta*w) + p*beta ;  p += r*1 ;  [y = M^-1 p]
template <class T, class V, bool PC>
struct BicgK1 {
    BicgState<T> *S; const Real<T> *partN; const T *partRho; int P; int mode;
    const T *v; const T *r; T *p; const V *dinv; T *y;
    T a, beta;
    unsigned int tag = 0; unsigned long long mb_timeout = 0;     // peer-to-peer hand-off: partN = this rank's mailbox entries, P = world (device.hpp, mbox_sum2)
    __device__ __forceinline__ bool prologue() {
        __shared__ Real<T> smD[NWAVE];
        __shared__ T smT[NWAVE];
        // every load of the prologue is issued before any is consumed (state words, then both partial arrays): one
        // memory round trip where the literal order (status -> |r| partials -> tol -> rho partials -> ...) paid four.
        // Only fields that no workgroup of THIS launch writes are read (rho / r_norm / beta are written below).
        const int status = S->status;
        const Real<T> tol2 = S->tol2, r0_norm_tol = S->r0_norm_tol;
        const T w = S->w, rho_old = S->rho_old, alpha = S->alpha;
        T rho; Real<T> r_norm;
        if (mode == 0) {
            Real<T> sN; T sR;
            if (tag != 0) {                                          // (status first: a stopped solve's producers posted nothing)
                if (status != ST_RUNNING) return false;
                if (!mbox_sum2(MboxSrc{reinterpret_cast<const unsigned long long *>(partN), P, tag, mb_timeout}, sN, sR)) {
                    if (first_thread()) S->status = ST_COMM_TIMEOUT;
                    return false;
                }
            } else {
                reduce_partials2(partN, partRho, P, smD, smT, sN, sR);  // :123 |r|^2, :128 r0.r
                if (status != ST_RUNNING) return false;
            }
            r_norm = ssqrt(sN);                                      // :123
            if (r_norm <= tol2) {                                    // :124
                if (first_thread()) { S->r_norm = r_norm; S->status = ST_CONVERGED; }
                return false;
            }
            rho = sR;                                                // :128
            if (sabs(rho) < r0_norm_tol) {                           // :131 -> host runs :132-145
                if (first_thread()) { S->r_norm = r_norm; S->status = ST_RESTART; }
                return false;
            }
        } else {  // resumed after the host-side restart: rho, r0_norm_tol already updated
            if (status != ST_RUNNING) return false;
            rho = S->rho; r_norm = S->r_norm;
        }
        beta = smul(sdiv(rho, rho_old), sdiv(alpha, w));             // :146
        a = smul(sneg(beta), w);                                     // :155  -beta * w
        if (first_thread()) { S->rho = rho; S->r_norm = r_norm; S->beta = beta; }
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        auto vv = ldp<T, PK, NT>(v, i); auto pv = ldp<T, PK, NT>(p, i); auto rv = ldp<T, PK, NT>(r, i);
        Pack<T, PK> yv;
        [[maybe_unused]] Pack<V, PK> dv;
        if (PC) dv = ldp<V, PK, NT>(dinv, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            T t = sadd(smul(vv.v[e], a), smul(pv.v[e], beta));      // :155 axpby
            t = sadd(t, smul(rv.v[e], sone<T>()));                  // :156 axpy(one, r, p)
            pv.v[e] = t;
            if (PC) yv.v[e] = smulv(t, dv.v[e]);                    // :328
        }
        stp<T, PK, NT>(p, i, pv);
        if (PC) stp<T, PK, NT>(y, i, yv);
    }
    __device__ __forceinline__ void epilogue() const {}
};

// K3  bicg_stab.rs:163-172 (+ :343):  alpha = rho / (r0.v) ; r -= alpha*v ; [z = M^-1 r]
template <class T, class V, bool PC>
struct BicgK3 {
    BicgState<T> *S; const T *partB; int P; int check_breakdown;
    const T *v; T *r; const V *dinv; T *z;
    T na;
    unsigned int tag = 0; unsigned long long mb_timeout = 0;     // peer-to-peer hand-off (see BicgK1)
    __device__ __forceinline__ bool prologue() {
        __shared__ T smT[NWAVE];
        const int status = S->status;                               // requested together with the partials
        const T rho = S->rho;
        T tmp;
        if (tag != 0) {
            if (status != ST_RUNNING) return false;
            if (!mbox_sum1(MboxSrc{reinterpret_cast<const unsigned long long *>(partB), P, tag, mb_timeout}, tmp)) {
                if (first_thread()) S->status = ST_COMM_TIMEOUT;
                return false;
            }
        } else {
            tmp = reduce_partials(partB, P, smT);                   // :163
            if (status != ST_RUNNING) return false;
        }
        if (check_breakdown && sabs(tmp) <= 0.0) {                  // :164-167
            if (first_thread()) S->status = ST_BREAKDOWN;
            return false;
        }
        const T alpha = sdiv(rho, tmp);                             // :169
        na = sneg(alpha);
        if (first_thread()) S->alpha = alpha;
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        auto vv = ldp<T, PK, NT>(v, i); auto rv = ldp<T, PK, NT>(r, i);
        Pack<T, PK> zv;
        [[maybe_unused]] Pack<V, PK> dv;
        if (PC) dv = ldp<V, PK, NT>(dinv, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            rv.v[e] = sadd(rv.v[e], smul(vv.v[e], na));             // :172
            if (PC) zv.v[e] = smulv(rv.v[e], dv.v[e]);              // :343
        }
        stp<T, PK, NT>(r, i, rv);
        if (PC) stp<T, PK, NT>(z, i, zv);
    }
    __device__ __forceinline__ void epilogue() const {}
};

// ---- spmv_chain.hip: the chain SpMV with the preceding vector update formed on the fly (f64, no preconditioner, single GPU)
// K3 into K4 (bicg_stab.rs:163-178):  alpha from partB (pro's prologue) ; s = r + v * (-alpha), formed on the fly and — s_out ==
//   nullptr — not stored (the pair2 walk of the blocks outside the chains honours a non-null s_out) ; t = A s ; partials of t.t and t.s.
//   store_t = false: t is not stored either (the same launch with the y store compiled out: K5 on the chains folds t again)
int launch_chain_k4f(const sprs_csr *A, const SpmvRoute &rt, const BicgK3<double, double, false> &pro, const double *r, const double *v, double *s_out,
                     double *t, double *partTT, double *partTR, const int *status, bool store_t = true);
// K1 into K2 (bicg_stab.rs:123-163):  norm / convergence / restart / beta (pro's prologue) ; p' = (v * (-beta w) + p * beta) + r -> p_out ;
//   v' = A p' -> v_out ; partials of r0.v'
int launch_chain_k2f(const sprs_csr *A, const SpmvRoute &rt, const BicgK1<double, double, false> &pro, const double *v_old, const double *p, const double *r,
                     double *p_out, double *v_out, const double *r0, double *partB, const int *status);

// K5  bicg_stab.rs:178-196:  w = (t.t > 0) ? t.r / t.t : 0 ; x -= alpha*y ; x -= w*s ; r -= w*t
//     + partials of norm2(r)^2 and r0.r for the next iteration's K1 (:123,:128)
// SV (fused SpMV input, bicgstab.hip): K4 formed s = r + v (-alpha) on the fly and did NOT store it — a store of s costs the fused K4
// 80 of its 294 us (scripts/micro/fused_window.hip, profiles/r04_tuning.md §3) — so s is formed again here from r and v with the
// same expression (K3's, bicg_stab.rs:172): one more read, which finds r and v in the Infinity Cache behind K4's reads; r' = s - w t
// is written over r.
template <class T, bool PC, bool SV = false>
struct BicgK5 {
    BicgState<T> *S; const T *partTT; const T *partTR; int P;
    const T *y; const T *z; const T *t; const T *r0; T *x; T *r; Real<T> *partN; T *partRho;
    Fin fin;                    // distributed: the last workgroup reduces (partN, partRho) for the all-reduce
    T na, nw, w;
    Real<T> accN; T accR;
    unsigned int tag = 0; unsigned long long mb_timeout = 0;     // peer-to-peer hand-off (see BicgK1): partTT = this rank's mailbox entries
    const T *sv = nullptr;                                       // SV: the v of s = r + v (-alpha)
    __device__ __forceinline__ bool prologue() {
        __shared__ T smT[NWAVE];
        __shared__ T smT2[NWAVE];
        const int status = S->status;                               // requested together with the partials
        const T alpha = S->alpha;
        T tt, tr;
        if (tag != 0) {
            if (status != ST_RUNNING) { fin_idle(fin, true); return false; }
            if (!mbox_sum2(MboxSrc{reinterpret_cast<const unsigned long long *>(partTT), P, tag, mb_timeout}, tt, tr)) {
                if (first_thread()) S->status = ST_COMM_TIMEOUT;
                return false;
            }
        } else {
            reduce_partials2(partTT, partTR, P, smT, smT2, tt, tr); // :178, :183
        }
        if (status != ST_RUNNING) { fin_idle(fin, true); return false; }
        w = (sre(tt) > 0.0) ? sdiv(tr, tt) : szero<T>();            // :179-186
        na = sneg(alpha); nw = sneg(w);
        accN = 0.0; accR = szero<T>();
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto xv = ldp<T, PK, NT>(x, i); auto yv = ldp<T, PK, NT>(y, i); auto rv = ldp<T, PK, NT>(r, i);
        auto tv = ldp<T, PK, NT>(t, i); auto qv = ldp<T, PK, NT>(r0, i);
        [[maybe_unused]] Pack<T, PK> zv;
        if (PC) zv = ldp<T, PK, NT>(z, i);
        if constexpr (SV) {
            const auto vv = ldp<T, PK, NT>(sv, i);
#pragma unroll
            for (int e = 0; e < PK; ++e) rv.v[e] = sadd(rv.v[e], smul(vv.v[e], na));    // :172  s = r - alpha v (K3's expression)
        }
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            T xx = sadd(xv.v[e], smul(yv.v[e], na));                // :188
            xx = sadd(xx, smul(PC ? zv.v[e] : rv.v[e], nw));        // :191 / :357
            xv.v[e] = xx;
            const T rr = sadd(rv.v[e], smul(tv.v[e], nw));          // :196
            rv.v[e] = rr;
            accN = accN + ssq(rr);
            accR = sadd(accR, smul(sconj(qv.v[e]), rr));
        }
        stp<T, PK, NT>(x, i, xv);
        stp<T, PK, NT>(r, i, rv);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ Real<T> smD[NWAVE];
        __shared__ T smT[NWAVE];
        const Real<T> sN = block_sum(accN, smD);
        const T sR = block_sum(accR, smT);
        if (threadIdx.x == 0) { st_partial(fin, partN + blockIdx.x, sN); st_partial(fin, partRho + blockIdx.x, sR); }
        if (first_thread()) { S->w = w; S->rho_old = S->rho; S->its = S->its + 1; }
        if (fin.counter) finalize_last_block<Real<T>, T>(fin, true, smD, smT);
    }
};

// K5 on the chains (bicgstab.hip, knob "bicg_k5"; spmv_chain.hip UPD): pro's prologue and epilogue, s = pro.r + pro.sv (-alpha) staged in
//   the windows, t = A s folded again for the workgroup's rows (recompute) or loaded from pro.t, x updated in place, r' = s - w t -> r_out
//   (not pro.r: other workgroups still read its windows) ; one partial of |r'|^2 and of r0.r' per workgroup of the SpMV grid
int launch_chain_k5(const sprs_csr *A, const SpmvRoute &rt, const BicgK5<double, false, true> &pro, double *r_out, bool recompute);

}  // namespace sprs
