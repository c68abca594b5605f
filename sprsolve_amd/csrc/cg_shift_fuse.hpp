// Multi-shift conjugate gradients: the vector kernels of CgShift<T> (cg_shift.hip).  One CG run on A (the "seed", x_0 = 0)
// carries the solutions of (A + sigma_j I) x_j = rhs for m <= 8 shifts: the shifted residuals stay collinear with the seed's,
// r_j = zeta_j r, so every column needs only a scalar recurrence on zeta_j and its own x_j, p_j (the recurrence is stated in the
// header, sprs_cgshift_*).  A fused iteration is three launches whatever m is:
//   CA         q = A p with the partials of conj(p).q                                  (KrylovBase::spmv, any SpMV route)
//   CgShiftSB  alpha = rho / (p.q) ; zeta_j^(n+1) for every running column ; r += q (-alpha) ; partials of |r|^2
//   CgShiftSC  |r|, beta = |r|^2 / rho ; alpha_j, beta_j, convergence per column ; one pass over r, p and the active columns:
//              x_j += p_j alpha_j ; p_j = r zeta_j^(n+1) + p_j beta_j ; p = r 1 + p beta
// SC reads r, p and 2 m_active column vectors and writes p and 2 m_active: r's pack is loaded once for all columns.  The x update
// sits in SC, not SB: in SB it would read the P block a second time per iteration.
//
// Layout: X and P are column-major blocks, column j at base + j * stride with a stride that keeps every column 16-byte aligned
// (P: the work vectors' stride; X: the caller's m contiguous vectors of n where those are aligned, else a work block that is
// copied out once).  The per-column coefficients are the same in every lane: they are kept wave-uniform (sc_uniform) and the
// eight column slots are unrolled under a uniform `mask & (1 << j)` branch — no per-lane select and no dynamically indexed
// register array (cg_many_fuse.hpp says why that ends in scratch memory).  All loads of a trip are issued before any is consumed.
//
// State rules (CgShiftState), those of CgState / CgManyState:
//   * every workgroup re-reduces the producer's partials in the same fixed order => the same bits in every workgroup; workgroup
//     0's first thread records the results.
//   * A launch reads only fields that none of its workgroups writes.  The iteration number n is a kernel argument (the host's
//     count: every column shares the seed's).  zeta is a RING of three rows indexed by iteration: zeta_j^(k) lives in row k % 3,
//     SB of iteration n reads rows n % 3 and (n - 1) % 3 and writes row (n + 1) % 3, SC reads rows n % 3 and (n + 1) % 3 and
//     writes none.  SB reads run_mask (SC's) and writes act_mask and act_it; SC reads those two and writes run_mask; rho_prev
//     is rho as SB read it; a_prev, b_prev (re alpha_{n-1}, re beta_{n-1}) are read by SB and written by SC; col_status, its
//     and res are only written.  The one exception is CgKB's, and SB alone makes it: the status word is written by its
//     workgroup 0 from values every workgroup computes for itself, and a workgroup that sees the new value does what it would
//     have done anyway (nothing).  SC, which ends the solve while it still has x to advance, never reads the status word: it
//     runs iff SB of the same iteration ran (act_it == n, SB's alone to write).
//   * `status` is ST_RUNNING while a column runs; once it is not, every later launch, the SpMV included, returns at its first
//     instruction.  A column leaves the masks once (converged, or its zeta recurrence broke down) and is frozen from then on:
//     its x, p and zeta are neither read nor written.
//   * no atomics; every loop is bounded.
#pragma once
#include "fused_launch.hpp"

namespace sprs {

constexpr int CGS_MAXM = 8;
// `status` once no column runs; col_status beside ST_RUNNING / ST_CONVERGED / ST_BREAKDOWN
enum : int { CGS_DONE = 1, CGS_UNUSED = 17 };

template <class T>
struct CgShiftState {
    T rho, rho_prev, alpha, beta;
    Real<T> r_norm, tol2, rhs_norm, pad0;
    double a_prev, b_prev;                  // re(alpha_{n-1}), re(beta_{n-1}) of the seed
    double sigma[CGS_MAXM];
    double zeta[3][CGS_MAXM];               // the ring: zeta_j^(k) in row k % 3
    Real<T> res[CGS_MAXM];                  // |zeta_j| |r| / |rhs| at the column's convergence
    long long its[CGS_MAXM];                // the column's event: completed iterations
    int col_status[CGS_MAXM];
    long long act_it;                       // the iteration whose SB wrote act_mask (-1: none yet)
    int status, run_mask, act_mask, pad1;   // run_mask: columns running after SC; act_mask: columns this iteration advances
};

// a value that is the same in every lane, moved to scalar registers
__device__ __forceinline__ int sc_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float sc_uniform(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ double sc_uniform(double v) {
    const long long b = __builtin_bit_cast(long long, v);
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)b);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(b >> 32));
    return __builtin_bit_cast(double, (long long)(((unsigned long long)hi << 32) | lo));
}

// SB:  pq = conj(p).q ; positive?  alpha = rho / pq, a = re(alpha) ; for every running column, in double:
//          den = a b_prev (zeta_prev - zeta) + zeta_prev a_prev (1 + sigma a) ; zeta_next = zeta zeta_prev a_prev / den
//      (den == 0 or zeta_next not finite: that column alone breaks down) ; r += q*(-alpha) + partials of |r|^2.
//      Reads r, q; writes r.  n = `it`.
template <class T>
struct CgShiftSB {
    CgShiftState<T> *S; const T *partPQ; int P; int m; long long it;
    const T *q; T *r; Real<T> *partN;
    T na; Real<T> accN;
    __device__ __forceinline__ bool prologue() {
        __shared__ T smT[NWAVE];
        const int status = S->status;                               // requested together with the partials
        const T rho = S->rho;
        const int run = S->run_mask;
        const double a_prev = S->a_prev, b_prev = S->b_prev;
        const int cur = (int)(it % 3), prev = (int)((it + 2) % 3), nxt = (int)((it + 1) % 3);
        double zc[CGS_MAXM], zp[CGS_MAXM], sg[CGS_MAXM];
#pragma unroll
        for (int j = 0; j < CGS_MAXM; ++j) {
            zc[j] = 1.0; zp[j] = 1.0; sg[j] = 0.0;
            if (j < m) { zc[j] = S->zeta[cur][j]; zp[j] = S->zeta[prev][j]; sg[j] = S->sigma[j]; }
        }
        const T pq = reduce_partials(partPQ, P, smT);
        if (status != ST_RUNNING) return false;
        if (!(sre(pq) > 0.0)) {                                     // A is not positive definite along p (a NaN lands here too)
            if (first_thread()) {
#pragma unroll
                for (int j = 0; j < CGS_MAXM; ++j)
                    if (j < m && ((run >> j) & 1)) { S->col_status[j] = ST_BREAKDOWN; S->its[j] = it; }
                S->act_mask = 0; S->act_it = it; S->status = CGS_DONE;
            }
            return false;
        }
        const T alpha = sdiv(rho, pq);
        const double a = (double)sre(alpha);
        int act = 0;
#pragma unroll
        for (int j = 0; j < CGS_MAXM; ++j) {
            if (j < m && ((run >> j) & 1)) {
                const double den = a * b_prev * (zp[j] - zc[j]) + zp[j] * a_prev * (1.0 + sg[j] * a);
                const double zn = zc[j] * zp[j] * a_prev / den;
                const bool bad = den == 0.0 || !isfinite(zn);
                if (!bad) act |= 1 << j;
                if (first_thread()) {
                    if (bad) { S->col_status[j] = ST_BREAKDOWN; S->its[j] = it; }
                    else S->zeta[nxt][j] = zn;
                }
            }
        }
        if (first_thread()) {
            S->alpha = alpha; S->rho_prev = rho; S->act_mask = act; S->act_it = it;
            if (act == 0) S->status = CGS_DONE;
        }
        if (act == 0) return false;
        na = sneg(alpha);
        accN = 0.0;
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto rv = ldp<T, PK, NT>(r, i); const auto qv = ldp<T, PK, NT>(q, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            const T rr = sadd(rv.v[e], smul(qv.v[e], na));          // axpy(-alpha, q, r)
            rv.v[e] = rr;
            accN = accN + ssq(rr);
        }
        stp<T, PK, NT>(r, i, rv);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ Real<T> smD[NWAVE];
        const Real<T> sN = block_sum(accN, smD);
        if (threadIdx.x == 0) partN[blockIdx.x] = sN;
    }
};

// SC:  r_norm = sqrt(sum |r|^2) ; rho_new = sum |r|^2 ; beta = rho_new / rho, b = re(beta) ; for every column of act_mask, in
//      double:  t = zeta_next / zeta ; alpha_j = a t ; beta_j = b (t t) ; converged where |zeta_next| r_norm <= tol2.
//      One pass:  x_j += p_j*alpha_j (every column of act_mask) ; p_j = r*zeta_next + p_j*beta_j (those that go on) ;
//      p = r*1 + p*beta (while a column goes on).  alpha_j, zeta_next, beta_j are rounded to Real<T> and applied as smulv does.
//      X, PB: column j at + j * xs / + j * ps.  n = `it`.
template <class T>
struct CgShiftSC {
    CgShiftState<T> *S; const Real<T> *partN; int P; int m; long long it;
    const T *r; T *p; T *X; T *PB; int64_t xs, ps;
    int adv, cont;                          // uniform masks: columns whose x is advanced / whose p is too
    T one, beta;
    Real<T> ca[CGS_MAXM], cz[CGS_MAXM], cb[CGS_MAXM];
    __device__ __forceinline__ bool prologue() {
        __shared__ Real<T> smD[NWAVE];
        // only fields that no workgroup of THIS launch writes are read (rho, beta, r_norm, a_prev, b_prev, run_mask and status
        // are written below)
        const long long act_it = S->act_it;
        const int act = S->act_mask;
        const Real<T> tol2 = S->tol2, rhs_norm = S->rhs_norm;
        const T rho = S->rho_prev, alpha = S->alpha;
        const int cur = (int)(it % 3), nxt = (int)((it + 1) % 3);
        double zc[CGS_MAXM], zn[CGS_MAXM];
#pragma unroll
        for (int j = 0; j < CGS_MAXM; ++j) {
            zc[j] = 1.0; zn[j] = 1.0;
            if (j < m) { zc[j] = S->zeta[cur][j]; zn[j] = S->zeta[nxt][j]; }
        }
        const Real<T> sN = reduce_partials(partN, P, smD);
        if (act_it != it || act == 0) return false;                 // the solve ended before this iteration, or in its SB
        const Real<T> r_norm = ssqrt(sN);
        const T rho_new = sfromr<T>(sN);
        const T be = sdiv(rho_new, rho);
        const double a = (double)sre(alpha), b = (double)sre(be);
        int go = 0;
#pragma unroll
        for (int j = 0; j < CGS_MAXM; ++j) {
            ca[j] = 0.0; cz[j] = 0.0; cb[j] = 0.0;
            if (j < m && ((act >> j) & 1)) {
                const double t = zn[j] / zc[j];
                const double w = fabs(zn[j]) * (double)r_norm;
                const bool conv = w <= (double)tol2;
                ca[j] = sc_uniform((Real<T>)(a * t));
                cz[j] = sc_uniform((Real<T>)zn[j]);
                cb[j] = sc_uniform((Real<T>)(b * (t * t)));
                if (!conv) go |= 1 << j;
                if (first_thread() && conv) {
                    S->col_status[j] = ST_CONVERGED; S->its[j] = it + 1; S->res[j] = (Real<T>)(w / (double)rhs_norm);
                }
            }
        }
        if (first_thread()) {
            S->r_norm = r_norm; S->rho = rho_new; S->beta = be; S->a_prev = a; S->b_prev = b; S->run_mask = go;
            if (go == 0) S->status = CGS_DONE;
        }
        adv = sc_uniform(act); cont = sc_uniform(go);
        one = sone<T>(); beta = be;
        return adv != 0;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        Pack<T, PK> xv[CGS_MAXM], pv[CGS_MAXM];
#pragma unroll
        for (int j = 0; j < CGS_MAXM; ++j) {
            if (adv & (1 << j)) { xv[j] = ldp<T, PK, NT>(X + j * xs, i); pv[j] = ldp<T, PK, NT>(PB + j * ps, i); }
        }
        const auto rv = ldp<T, PK, NT>(r, i);
        Pack<T, PK> sv = rv;
        if (cont) sv = ldp<T, PK, NT>(p, i);
#pragma unroll
        for (int j = 0; j < CGS_MAXM; ++j) {
            if (adv & (1 << j)) {
#pragma unroll
                for (int e = 0; e < PK; ++e) xv[j].v[e] = sadd(xv[j].v[e], smulv(pv[j].v[e], ca[j]));           // axpy(alpha_j, p_j, x_j)
                stp<T, PK, NT>(X + j * xs, i, xv[j]);
                if (cont & (1 << j)) {
#pragma unroll
                    for (int e = 0; e < PK; ++e) pv[j].v[e] = sadd(smulv(rv.v[e], cz[j]), smulv(pv[j].v[e], cb[j]));   // axpby(zeta_j, r, beta_j, p_j)
                    stp<T, PK, NT>(PB + j * ps, i, pv[j]);
                }
            }
        }
        if (cont) {
#pragma unroll
            for (int e = 0; e < PK; ++e) sv.v[e] = sadd(smul(rv.v[e], one), smul(sv.v[e], beta));              // axpby(1, r, beta, p)
            stp<T, PK, NT>(p, i, sv);
        }
    }
    __device__ __forceinline__ void epilogue() const {}
};

}  // namespace sprs
