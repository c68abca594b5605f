// Conjugate gradients' two vector kernels (the solver itself: Cg<T> in cg.hip).  No reference analogue — the recurrence is
// the one stated in the header (sprs_cg_*), in the conventions of the library's BiCGStab.  A fused iteration is three launches:
//   CA    q = A p with the partials of conj(p).q                      (KrylovBase::spmv, any SpMV route)
//   CgKB  alpha = rho / (p.q) ; x += p alpha ; r += q (-alpha) ; [z = M^-1 r] ; partials of |r|^2 and conj(r).z
//   CgKC  r_norm, convergence ; rho_new, beta = rho_new / rho ; p = z 1 + p beta
// Both kernels follow BicgK1 / K3 / K5: the prologue re-reduces the producer's partials in every workgroup (same partials, same
// order => the same bits everywhere) with all its loads issued before any is consumed, workgroup 0 records the scalars, and once
// the status word leaves ST_RUNNING every later kernel returns at its first instruction.
#pragma once
#include "fused_launch.hpp"

namespace sprs {

// Device-resident scalar state of a CG solve.  `its` counts completed iterations = the 0-based index of the running one.
// rho_prev is rho as CgKB read it: CgKC writes rho, so its workgroups read the copy that no workgroup of their launch writes.
template <class T>
struct CgState {
    T rho, rho_prev, alpha, beta;
    Real<T> r_norm, tol2, pc_re, pad0;
    long long its;
    int status, pad1;
};

// KB:  pq = conj(p).q ; positive?  alpha = rho / pq ; x += p*alpha ; r += q*(-alpha) ; [z = M^-1 r]
//      + partials of norm2(r)^2 and conj(r).z for KC.  Reads x, p, r, q (+ dinv), writes x, r (+ z).
template <class T, class V, bool PC>
struct CgKB {
    CgState<T> *S; const T *partPQ; int P;
    const T *p; const T *q; T *x; T *r; const V *dinv; T *z; Real<T> *partN; T *partRZ;
    Fin fin;                    // distributed: the last workgroup reduces (partN, partRZ) for the all-reduce
    T alpha, na;
    Real<T> accN; T accR;
    __device__ __forceinline__ bool prologue() {
        __shared__ T smT[NWAVE];
        const int status = S->status;                               // requested together with the partials
        const T rho = S->rho;
        const T pq = reduce_partials(partPQ, P, smT);
        if (status != ST_RUNNING) { fin_idle(fin, true); return false; }
        if (!(sre(pq) > 0.0)) {                                     // A is not positive definite along p (a NaN lands here too)
            if (first_thread()) S->status = ST_BREAKDOWN;
            fin_idle(fin, true);
            return false;
        }
        alpha = sdiv(rho, pq);
        na = sneg(alpha);
        accN = 0.0; accR = szero<T>();
        if (first_thread()) { S->alpha = alpha; S->rho_prev = rho; }
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto xv = ldp<T, PK, NT>(x, i); auto pv = ldp<T, PK, NT>(p, i); auto rv = ldp<T, PK, NT>(r, i); auto qv = ldp<T, PK, NT>(q, i);
        [[maybe_unused]] Pack<T, PK> zv;
        [[maybe_unused]] Pack<V, PK> dv;
        if (PC) dv = ldp<V, PK, NT>(dinv, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            xv.v[e] = sadd(xv.v[e], smul(pv.v[e], alpha));          // axpy(alpha, p, x)
            const T rr = sadd(rv.v[e], smul(qv.v[e], na));          // axpy(-alpha, q, r)
            rv.v[e] = rr;
            T zz = rr;
            if (PC) { zz = smulv(rr, dv.v[e]); zv.v[e] = zz; }      // z = M^-1 r
            accN = accN + ssq(rr);
            accR = sadd(accR, smul(sconj(rr), zz));                 // conj_dot(r, z)
        }
        stp<T, PK, NT>(x, i, xv);
        stp<T, PK, NT>(r, i, rv);
        if (PC) stp<T, PK, NT>(z, i, zv);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ Real<T> smD[NWAVE];
        __shared__ T smT[NWAVE];
        const Real<T> sN = block_sum(accN, smD);
        const T sR = block_sum(accR, smT);
        if (threadIdx.x == 0) { st_partial(fin, partN + blockIdx.x, sN); st_partial(fin, partRZ + blockIdx.x, sR); }
        if (fin.counter) finalize_last_block<Real<T>, T>(fin, true, smD, smT);
    }
};

// KC:  r_norm = sqrt(sum |r|^2) ; converged?  rho_new = conj(r).z ; positive (preconditioned)?  beta = rho_new / rho ;
//      p = z*1 + p*beta.  Reads z (= r without a preconditioner) and p, writes p.
template <class T, bool PC>
struct CgKC {
    CgState<T> *S; const Real<T> *partN; const T *partRZ; int P;
    const T *z; T *p;
    T one, beta;
    __device__ __forceinline__ bool prologue() {
        __shared__ Real<T> smD[NWAVE];
        __shared__ T smT[NWAVE];
        // only fields that no workgroup of THIS launch writes are read (rho, beta, r_norm, its are written below)
        const int status = S->status;
        const Real<T> tol2 = S->tol2;
        const T rho = S->rho_prev;
        Real<T> sN; T rho_new;
        reduce_partials2(partN, partRZ, P, smD, smT, sN, rho_new);
        if (status != ST_RUNNING) return false;
        const Real<T> r_norm = ssqrt(sN);
        if (r_norm <= tol2) {
            if (first_thread()) { S->r_norm = r_norm; S->its = S->its + 1; S->status = ST_CONVERGED; }
            return false;
        }
        if (PC && !(sre(rho_new) > 0.0)) {
            if (first_thread()) { S->r_norm = r_norm; S->pc_re = sre(rho_new); S->status = ST_INVALID_PC; }
            return false;
        }
        beta = sdiv(rho_new, rho);
        one = sone<T>();
        if (first_thread()) { S->rho = rho_new; S->beta = beta; S->r_norm = r_norm; S->its = S->its + 1; }
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        auto zv = ldp<T, PK, NT>(z, i); auto pv = ldp<T, PK, NT>(p, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) pv.v[e] = sadd(smul(zv.v[e], one), smul(pv.v[e], beta));   // axpby(1, z, beta, p)
        stp<T, PK, NT>(p, i, pv);
    }
    __device__ __forceinline__ void epilogue() const {}
};

// RZ (applied preconditioners only: ILU(0), AMG): z = P r is a chain of launches of its own between KB and KC, so KB runs
//      without a preconditioner and this pass forms the partials of conj(r).z that KC expects.  Reads r and z.
template <class T>
struct CgRZ {
    const CgState<T> *S; const T *r; const T *z; T *partRZ;
    T accR;
    __device__ __forceinline__ bool prologue() {
        if (S->status != ST_RUNNING) return false;
        accR = szero<T>();
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        const auto rv = ldp<T, PK, NT>(r, i); const auto zv = ldp<T, PK, NT>(z, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) accR = sadd(accR, smul(sconj(rv.v[e]), zv.v[e]));          // conj_dot(r, z)
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ T smT[NWAVE];
        const T sR = block_sum(accR, smT);
        if (threadIdx.x == 0) partRZ[blockIdx.x] = sR;
    }
};

}  // namespace sprs
