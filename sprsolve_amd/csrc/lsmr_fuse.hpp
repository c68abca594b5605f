// LSMR's scalar recurrence and its three vector kernels (the solver itself: Lsmr<T> in lsmr.hip).  No reference analogue — the
// recurrence is the one stated in the header (sprs_lsmr_*): Fong & Saunders' LSMR on the Golub-Kahan bidiagonalisation, every
// recurrence scalar real.  u (length m = rows) stays UN-NORMALISED in memory, u = beta u_k; each reader applies 1 / beta.
// A fused iteration is five launches:
//   SpMV  w = A v                                                                  (any SpMV route of A)
//   LsKU  [the stop tests of the previous iteration]  u = w + u f, f = -(alpha (1 / beta)) ; partials of |u|^2      3 passes of m
//   SpMV  w' = A^H u                                                               (any SpMV route of the adjoint handle)
//   LsKV  beta = |u| ; v = w' (1 / beta) + v (-beta) ; partials of |v|^2                                            3 passes of n
//   LsKH  alpha = |v| ; the plane rotations and norm estimates (ls_step) ; hbar = h + hbar g1 ; x += hbar g2 ;
//         v *= 1 / alpha ; h = v + h g3 ; partials of |x|^2                                                         8 passes of n
// The stop tests need |x| of the iteration just finished, which LsKH can only hand over as partials: they are taken by the next
// launch that runs — LsKU of the next iteration, or LsKT, the one-workgroup launch the host puts in front of every poll.  Both
// evaluate the same function of the same state and partials, so the event does not depend on `poll`.
// State rules (as CgState's): the scalars of an iteration boundary live in st[its & 1]; the kernels of iteration `its` read
// st[its & 1] and workgroup 0 of LsKH writes st[(its + 1) & 1], so no launch reads a word one of its workgroups writes; every
// workgroup re-reduces the same partials in the same order and takes the same decision; once the status word leaves ST_RUNNING
// every later launch returns at its first instruction.
#pragma once
#include "fused_launch.hpp"

namespace sprs {

// The scalars at an iteration boundary.  `its` counts completed iterations.
template <class R>
struct LsIter {
    R alpha, beta;                                   // alpha_k ; beta_k, the norm of u as it stands in memory
    R alphabar, zetabar, rho, rhobar, cbar, sbar;
    R betadd, betad, rhodold, tautildeold, thetatilde, zeta, d;
    R normA2, normA, normr, normar;
    R lucky;                                         // 1: the iteration that wrote this met beta = 0 or alpha = 0
    long long its;
};
template <class R>
struct LsDev {
    LsIter<R> st[2];
    R normb, tol, damp;                              // written by the host only
    R ev_res, ev_ares, pad0;                         // the event's |r| / |b| and |A^H r| / (|A| |r|)
    long long ev_its;
    int status, pad1;
};

template <class R> SPRS_HD bool ls_finite(R x) { return x - x == (R)0; }
template <class R> SPRS_HD R ls_sign(R x) { return x > (R)0 ? (R)1 : (x < (R)0 ? (R)-1 : (R)0); }
template <class R> SPRS_HD R ls_abs(R x) { return x < (R)0 ? -x : x; }

// the stable plane rotation: c a + s b = r, -s a + c b = 0
template <class R>
SPRS_HD void ls_symortho(R a, R b, R &c, R &s, R &r) {
    if (b == (R)0) { c = ls_sign(a); s = (R)0; r = ls_abs(a); }
    else if (a == (R)0) { c = (R)0; s = ls_sign(b); r = ls_abs(b); }
    else if (ls_abs(b) > ls_abs(a)) { const R tau = a / b; s = ls_sign(b) / ssqrt((R)1 + tau * tau); c = s * tau; r = b / s; }
    else { const R tau = b / a; c = ls_sign(a) / ssqrt((R)1 + tau * tau); s = c * tau; r = a / c; }
}

// One step of the scalar recurrence (header, steps S1 - S8): from the boundary `s` and the new beta, alpha to the boundary `o`
// and the factors of the vector updates.  false: a factor or a norm estimate is not finite.
template <class R>
SPRS_HD bool ls_step(const LsIter<R> &s, R damp, R beta, R alpha, LsIter<R> &o, R &g1, R &g2, R &g3) {
    R chat, shat, alphahat, c, sn, rho, cbar, sbar, rhobar, ctil, stil, rhotil;
    ls_symortho(s.alphabar, damp, chat, shat, alphahat);
    ls_symortho(alphahat, beta, c, sn, rho);
    const R thetanew = sn * alpha;
    o.alphabar = c * alpha;
    const R thetabar = s.sbar * rho;
    ls_symortho(s.cbar * rho, thetanew, cbar, sbar, rhobar);
    const R zeta = cbar * s.zetabar;
    o.zetabar = -sbar * s.zetabar;
    g1 = -(thetabar * rho / (s.rho * s.rhobar));
    g2 = zeta / (rho * rhobar);
    g3 = -(thetanew / rho);
    const R betaacute = chat * s.betadd, betacheck = -shat * s.betadd;
    const R betahat = c * betaacute;
    o.betadd = -sn * betaacute;
    ls_symortho(s.rhodold, thetabar, ctil, stil, rhotil);
    o.thetatilde = stil * rhobar;
    o.rhodold = ctil * rhobar;
    o.betad = -stil * s.betad + ctil * betahat;
    o.tautildeold = (s.zeta - s.thetatilde * s.tautildeold) / rhotil;
    const R taud = (zeta - o.thetatilde * o.tautildeold) / o.rhodold;
    o.d = s.d + betacheck * betacheck;
    const R dt = o.betad - taud;
    o.normr = ssqrt(o.d + dt * dt + o.betadd * o.betadd);
    const R a2 = s.normA2 + beta * beta;
    o.normA = ssqrt(a2);
    o.normA2 = a2 + alpha * alpha;
    o.normar = ls_abs(o.zetabar);
    o.rho = rho; o.rhobar = rhobar; o.cbar = cbar; o.sbar = sbar; o.zeta = zeta;
    o.alpha = alpha; o.beta = beta;
    o.lucky = (beta == (R)0 || alpha == (R)0) ? (R)1 : (R)0;
    o.its = s.its + 1;
    return ls_finite(g1) && ls_finite(g2) && ls_finite(g3) && ls_finite(o.normr) && ls_finite(o.normA) && ls_finite(o.normar);
}

// the stop tests at a boundary, with normx = |x|
template <class R>
SPRS_HD bool ls_converged(const LsIter<R> &s, R normb, R tol, R normx) {
    return s.lucky != (R)0 || s.normr <= tol * normb + tol * s.normA * normx || s.normar <= tol * s.normA * s.normr;
}
template <class R> SPRS_HD R ls_res(const LsIter<R> &s, R normb) { return s.normr / normb; }
template <class R> SPRS_HD R ls_ares(const LsIter<R> &s) { const R dn = s.normA * s.normr; return dn > (R)0 ? s.normar / dn : (R)0; }

// Two partial arrays of different lengths at once: every load is issued before any sum is formed and the two block sums share
// their barriers.  Per array the same per-thread addition order and the same wave / block order as reduce_partials.
template <class R>
__device__ __forceinline__ void ls_reduce2(const R *__restrict__ pa, int Pa, const R *__restrict__ pb, int Pb, R *smA, R *smB, R &ra, R &rb) {
    R a = (R)0, b = (R)0;
    for (int i = threadIdx.x; i < Pa; i += BLOCK) a = a + pa[i];
    for (int i = threadIdx.x; i < Pb; i += BLOCK) b = b + pb[i];
    a = wave_sum(a); b = wave_sum(b);
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { smA[wv] = a; smB[wv] = b; }
    __syncthreads();
    ra = smA[0]; rb = smB[0];
#pragma unroll
    for (int w = 1; w < NWAVE; ++w) { ra = ra + smA[w]; rb = rb + smB[w]; }
}

// The stop tests of the boundary st[par] with |x| from LsKH's partials.  true: the solve is over (now or before).
template <class R>
__device__ __forceinline__ bool ls_test(LsDev<R> *S, int par, const R *partX, int PX) {
    __shared__ R smX[NWAVE];
    const int status = S->status;                                   // requested together with the partials
    const LsIter<R> s = S->st[par];
    const R normb = S->normb, tol = S->tol;
    const R sx = reduce_partials(partX, PX, smX);
    if (status != ST_RUNNING) return true;
    if (s.its == 0) return false;                                   // no iteration has finished yet
    if (!ls_converged(s, normb, tol, ssqrt(sx))) return false;
    if (first_thread()) { S->ev_its = s.its; S->ev_res = ls_res(s, normb); S->ev_ares = ls_ares(s); S->status = ST_CONVERGED; }
    return true;
}

// LsKT: the stop tests alone (one workgroup, no vector), in front of a poll
template <class T>
struct LsKT {
    LsDev<Real<T>> *S; int par; const Real<T> *partX; int PX;
    static constexpr bool whole_packs = true;
    __device__ __forceinline__ bool prologue() { (void)ls_test(S, par, partX, PX); return false; }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t) const {}
    __device__ __forceinline__ void epilogue() const {}
};

// LsKU:  u = w + u*f, f = -(alpha * (1 / beta)) ; partials of |u|^2.  Reads w, u; writes u.
template <class T>
struct LsKU {
    using R = Real<T>;
    LsDev<R> *S; int par; const R *partX; int PX;
    const T *w; T *u; R *partU; Fin fin;
    R f, acc;
    __device__ __forceinline__ bool prologue() {
        if (ls_test(S, par, partX, PX)) return false;
        const R alpha = S->st[par].alpha, beta = S->st[par].beta;
        f = -(alpha * ((R)1 / beta));
        acc = (R)0;
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto wv = ldp<T, PK, NT>(w, i); auto uv = ldp<T, PK, NT>(u, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            uv.v[e] = sadd(wv.v[e], smulr(uv.v[e], f));
            acc = acc + ssq(uv.v[e]);
        }
        stp<T, PK, NT>(u, i, uv);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ R smD[NWAVE];
        const R s = block_sum(acc, smD);
        if (threadIdx.x == 0) st_partial(fin, partU + blockIdx.x, s);
        if (fin.counter) finalize_last_block<R, R>(fin, false, smD, smD);
    }
};

// LsKV:  beta = sqrt(sum |u|^2) ; finite?  zero (then v is left alone: LsKH ends the solve)?  v = w'*(1 / beta) + v*(-beta) ;
//        partials of |v|^2.  Reads w', v; writes v.
template <class T>
struct LsKV {
    using R = Real<T>;
    LsDev<R> *S; int par; const R *partU; int PU;
    const T *w; T *v; R *partV; Fin fin;
    R rb, nb, acc;
    __device__ __forceinline__ bool prologue() {
        __shared__ R smD[NWAVE];
        const int status = S->status;
        const long long its = S->st[par].its;
        const R b2 = reduce_partials(partU, PU, smD);
        if (status != ST_RUNNING) return false;
        const R beta = ssqrt(b2);
        if (!ls_finite(beta)) {
            if (first_thread()) { S->ev_its = its; S->status = ST_BREAKDOWN; }
            return false;
        }
        if (beta == (R)0) return false;
        rb = (R)1 / beta; nb = -beta; acc = (R)0;
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto wv = ldp<T, PK, NT>(w, i); auto vv = ldp<T, PK, NT>(v, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            vv.v[e] = sadd(smulr(wv.v[e], rb), smulr(vv.v[e], nb));
            acc = acc + ssq(vv.v[e]);
        }
        stp<T, PK, NT>(v, i, vv);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ R smD[NWAVE];
        const R s = block_sum(acc, smD);
        if (threadIdx.x == 0) st_partial(fin, partV + blockIdx.x, s);
        if (fin.counter) finalize_last_block<R, R>(fin, false, smD, smD);
    }
};

// LsKH:  beta, alpha from the partials ; ls_step ; hbar = h + hbar*g1 ; x = x + hbar*g2 ; v = v*(1 / alpha) ; h = v + h*g3 ;
//        partials of |x|^2.  Reads v, h, hbar, x and writes all four.
template <class T>
struct LsKH {
    using R = Real<T>;
    LsDev<R> *S; int par; const R *partU; int PU; const R *partV; int PV;
    T *v; T *h; T *hbar; T *x; R *partX; Fin fin;
    R g1, g2, g3, ra, acc;
    __device__ __forceinline__ bool prologue() {
        __shared__ R smA[NWAVE];
        __shared__ R smB[NWAVE];
        const int status = S->status;
        const LsIter<R> s = S->st[par];
        const R damp = S->damp;
        R b2, a2;
        ls_reduce2(partU, PU, partV, PV, smA, smB, b2, a2);
        if (status != ST_RUNNING) return false;
        const R beta = ssqrt(b2);
        const R alpha = beta == (R)0 ? (R)0 : ssqrt(a2);          // beta = 0: LsKV wrote no partials
        LsIter<R> o;
        if (!ls_finite(alpha) || !ls_step(s, damp, beta, alpha, o, g1, g2, g3)) {
            if (first_thread()) { S->ev_its = s.its; S->status = ST_BREAKDOWN; }
            return false;
        }
        ra = alpha > (R)0 ? (R)1 / alpha : (R)1;
        acc = (R)0;
        if (first_thread()) S->st[par ^ 1] = o;
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto vv = ldp<T, PK, NT>(v, i); auto hv = ldp<T, PK, NT>(h, i); auto bv = ldp<T, PK, NT>(hbar, i); auto xv = ldp<T, PK, NT>(x, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            bv.v[e] = sadd(hv.v[e], smulr(bv.v[e], g1));            // axpby(1, h, g1, hbar)
            xv.v[e] = sadd(xv.v[e], smulr(bv.v[e], g2));            // axpy(g2, hbar, x)
            vv.v[e] = smulr(vv.v[e], ra);                           // rscale(1 / alpha, v)
            hv.v[e] = sadd(vv.v[e], smulr(hv.v[e], g3));            // axpby(1, v, g3, h)
            acc = acc + ssq(xv.v[e]);
        }
        stp<T, PK, NT>(hbar, i, bv);
        stp<T, PK, NT>(x, i, xv);
        stp<T, PK, NT>(v, i, vv);
        stp<T, PK, NT>(h, i, hv);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ R smD[NWAVE];
        const R s = block_sum(acc, smD);
        if (threadIdx.x == 0) st_partial(fin, partX + blockIdx.x, s);
        if (fin.counter) finalize_last_block<R, R>(fin, false, smD, smD);
    }
};

}  // namespace sprs
