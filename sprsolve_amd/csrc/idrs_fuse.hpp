// IDR(s): the vector kernels of Idrs<T> (idrs.hip).  No reference analogue — the recurrence is the one stated in the header
// (sprs_idrs_*).  A cycle is s inner steps and one omega step, s + 1 products with A.  Inner step k:
//   IdrsA     |r| from the previous launch's partials, the step's events, c from M[k:,k:] c = f[k:] ; one pass over r, g_k .. g_{s-1},
//             u_k .. u_{s-1}:  v = r - sum c_i g_i ; u_k = (P v) omega + sum c_i u_i.  v is not stored with no preconditioner or a
//             diagonal one (applied in the pass).  An applied P: IdrsA<2> writes v, the handle's launches form vh = P v, IdrsA2
//             forms u_k in a second short pass.
//   SpMV      g_k = A u_k                                                 (KrylovBase::spmv, any route)
//   IdrsDots  partials of q = P^H g_k: ONE read of g_k per idrs_b<T> columns (GmDots' shape; 8 double accumulators, 4 complex ones)
//   IdrsB     q, alpha from M[:k,:k] alpha = q[:k], M's column k, beta, the new f ; one pass over g_k, u_k, g_i, u_i (i < k), r, x:
//             g_k -= sum alpha_i g_i ; u_k -= sum alpha_i u_i ; r -= beta g_k ; x += beta u_k ; partials of |r|^2
// and the omega step:
//   idrs_check (one workgroup) |r|, the events of step s - 1
//   [IdrsPrec vh = P r, or an applied P's launches]
//   SpMV      t = A vh with the partials of conj(t).t and conj(t).r (f64 / c64 ; f32 / c32: an IdrsDots launch on t against r and t)
//   IdrsW     omega ; x += omega vh ; r -= omega t ; partials of |r|^2 and of the next f = P^H r from the updated r (the complex
//             types: f is an IdrsDots launch of its own, idrs_fuse_f below)
// The conventions are gmres_fuse.hpp's: a consumer re-reduces its producer's partials in its prologue (same partials, same order
// in every workgroup => the same bits everywhere), workgroup 0 records the scalars, and the host reads nothing but the head.
// The small quantities (M, f, c, alpha, beta, q, omega) are kept and computed in double — complex double for a complex T — by
// thread 0 of every workgroup in LDS, in the header's order, and rounded to T where they multiply vectors; the pass reads them
// from LDS, the same in every lane.  "Computed in double" includes the sums: every dot product and |r|^2 of the recurrence is
// accumulated in double from exact products (dbl_cmul), so in f32 / c32 too the scalars do not depend on the summation order.  Every loop of the small solves is bounded by s <= 8.
//
// State rules (IdrsState):
//   * A launch reads only fields that none of its workgroups writes.  The step k and the product count `it` are kernel
//     arguments (the host's count).  f is indexed by step: F[k] is f as step k finds it; IdrsA of step 0 writes F[0] from the
//     partials (and reads the partials, not F[0]), IdrsB of step k reads F[k] and writes F[k + 1].  IdrsB of step k reads M's
//     columns < k and writes column k; IdrsA reads M and writes none of it.  omega is written by IdrsW, which does not read it.
//     hd.r_norm is written by the launches that take the step's events (IdrsA, idrs_check) and read by IdrsW.
//     The one exception is CgKB's: `status` is written by workgroup 0 from values every workgroup computes for itself, and a
//     workgroup that sees the new value does what it would have done anyway (nothing).
//   * `status` and `skip` leave zero together, once; every later kernel (the SpMV and IdrsDots included) then returns at its
//     first instruction, so x, r and its are those of the event.  An applied preconditioner's launches are not keyed on it:
//     they write vh and the handle's scratch only.
//   * no atomics.
#pragma once
#include <type_traits>

#include "gmres_fuse.hpp"

namespace sprs {

constexpr int IDRS_MAXS = SPRS_IDRS_MAX_S;
constexpr double IDRS_KAPPA = 0.7;

// the type of the small quantities
template <class T> using Dbl = std::conditional_t<is_complex<T>::value, cplx, double>;
SPRS_HD double to_dbl(double a) { return a; }
SPRS_HD double to_dbl(float a) { return (double)a; }
SPRS_HD cplx to_dbl(cplx a) { return a; }
SPRS_HD cplx to_dbl(cplxf a) { return cplx{(double)a.re, (double)a.im}; }
template <class T> SPRS_HD T from_dbl(Dbl<T> a);
template <> SPRS_HD double from_dbl<double>(double a) { return a; }
template <> SPRS_HD float from_dbl<float>(double a) { return (float)a; }
template <> SPRS_HD cplx from_dbl<cplx>(cplx a) { return a; }
template <> SPRS_HD cplxf from_dbl<cplxf>(cplx a) { return cplxf{(float)a.re, (float)a.im}; }
SPRS_HD bool dbl_finite(double a) { return isfinite(a); }
SPRS_HD bool dbl_finite(cplx a) { return isfinite(a.re) && isfinite(a.im); }
SPRS_HD bool dbl_is_zero(double a) { return a == 0.0; }
SPRS_HD bool dbl_is_zero(cplx a) { return a.re == 0.0 && a.im == 0.0; }

// IdrsW leaves the partials of the next f = P^H r itself where 8 double accumulators and 8 loads of P fit beside its four
// streams: the real types (a complex-double accumulator is 16 bytes: gm_b's spill case; DESIGN §4q has the registers)
template <class T> struct idrs_fuse_f { static constexpr bool value = !is_complex<T>::value; };
// columns per IdrsDots launch = accumulators per lane: 8, and 4 where they are complex double
template <class T> struct idrs_b { static constexpr int value = is_complex<T>::value ? 4 : 8; };
// conj(a) b in the type of the small quantities: for f32 / c32 the operands are widened first, so every product is exact and only
// the (double) sum rounds — the dot products of the recurrence do not depend on the summation order beyond 1e-16
SPRS_HD double dbl_cmul(double a, double b) { return a * b; }
SPRS_HD double dbl_cmul(float a, float b) { return (double)a * (double)b; }
SPRS_HD cplx dbl_cmul(cplx a, cplx b) { return smul(sconj(a), b); }
SPRS_HD cplx dbl_cmul(cplxf a, cplxf b) { return smul(sconj(to_dbl(a)), to_dbl(b)); }
SPRS_HD double dbl_sq(double a) { return a * a; }
SPRS_HD double dbl_sq(float a) { return (double)a * (double)a; }
SPRS_HD double dbl_sq(cplx a) { return a.re * a.re + a.im * a.im; }
SPRS_HD double dbl_sq(cplxf a) { return (double)a.re * (double)a.re + (double)a.im * (double)a.im; }

// What the host reads (every poll_interval() products) ...
template <class T>
struct IdrsHead {
    long long its, max_iter;    // its: products with A completed
    int status, skip;           // skip = (status != ST_RUNNING), set together
    int kind, pad0;             // the last step: k, or s for the omega step
    double r_norm, tol2, r0sq, pad1;    // r_norm: |r| as the last step found it ; r0sq: |r_0|^2, the host's
    double tr[4];               // the last step's trace row: its coefficient (beta / omega) and pivot (M_kk / tt)
};
// ... and the rest of the device-resident scalar state
template <class T>
struct IdrsState {
    IdrsHead<T> hd;
    Dbl<T> omega;
    Dbl<T> c[IDRS_MAXS];                        // an applied preconditioner: IdrsA's c for IdrsA2
    Dbl<T> F[IDRS_MAXS + 1][IDRS_MAXS];         // F[k]: f as step k finds it
    Dbl<T> M[IDRS_MAXS][IDRS_MAXS];             // M[i][j], lower triangular
};

// The events a step begins with, from |r|^2: every workgroup computes them, workgroup 0 records them.  False: the solve is over.
template <class T>
__device__ __forceinline__ bool idrs_decide(IdrsHead<T> *H, double sN, double tol2, long long max_iter, long long it) {
    const double rn = sqrt(sN);
    int ev = ST_RUNNING;
    if (!isfinite(rn)) ev = ST_BREAKDOWN;
    else if (rn <= tol2) ev = ST_CONVERGED;
    else if (it >= max_iter) ev = ST_MAX_ITER;
    if (first_thread()) {
        H->r_norm = rn;
        if (ev != ST_RUNNING) { H->its = it; H->skip = 1; H->status = ev; }
    }
    return ev == ST_RUNNING;
}

// ---- IdrsA: step k's first half.  MODE 0: no preconditioner ; 1: a diagonal, applied in the pass ; 2: an applied one — `out` is
// v and IdrsA2 follows.  PN == 0: the first step of a solve, |r|^2 is the host's r0sq.  partF (k == 0 only): s sums of PF partials.
template <class T, class V, int MODE>
struct IdrsA {
    IdrsState<T> *S; const double *partN; int PN; const Dbl<T> *partF; int64_t fstride; int PF; int s, k; long long it;
    const T *r; const T *Gb; const T *Ub; int64_t vs; const V *dinv; T *out;
    const T *cf; T om;
    __device__ __forceinline__ bool prologue() {
        using D = Dbl<T>;
        __shared__ double smD[NWAVE];
        __shared__ D fsum[IDRS_MAXS];
        __shared__ D sM[IDRS_MAXS * IDRS_MAXS], sf[IDRS_MAXS], sc[IDRS_MAXS];
        __shared__ T scT[IDRS_MAXS];
        __shared__ int s_status;                                    // one read a workgroup: every wavefront takes the same way
        IdrsHead<T> &H = S->hd;
        const double tol2 = H.tol2, r0sq = H.r0sq;
        const long long max_iter = H.max_iter;
        const D omega = S->omega;
        const int tid = threadIdx.x;
        if (tid == 0) s_status = H.status;                          // requested together with the partials
        if (tid < IDRS_MAXS * IDRS_MAXS) sM[tid] = (&S->M[0][0])[tid];
        if (k > 0 && tid < IDRS_MAXS) sf[tid] = S->F[k][tid];
        const double sN = PN > 0 ? reduce_partials(partN, PN, smD) : r0sq;
        if (k == 0) {
            reduce_coefs(partF, fstride, PF, s, fsum);
            if (tid < s) sf[tid] = fsum[tid];
        }
        __syncthreads();
        if (s_status != ST_RUNNING) return false;
        if (!idrs_decide<T>(&H, sN, tol2, max_iter, it)) return false;
        if (tid == 0) {
            for (int i = k; i < s; ++i) {                           // M[k:,k:] c = f[k:], forward
                D t = sf[i];
                for (int j = k; j < i; ++j) t = ssub(t, smul(sM[i * IDRS_MAXS + j], sc[j]));
                sc[i] = sdiv(t, sM[i * IDRS_MAXS + i]);
                scT[i] = from_dbl<T>(sc[i]);
            }
        }
        __syncthreads();
        if (blockIdx.x == 0 && tid < s) {
            if (k == 0) S->F[0][tid] = sf[tid];
            if (MODE == 2 && tid >= k) S->c[tid] = sc[tid];
        }
        cf = scT; om = from_dbl<T>(omega);
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        auto vv = ldp<T, PK, NT>(r, i);
        [[maybe_unused]] Pack<V, PK> dv;
        if constexpr (MODE == 1) dv = ldp<V, PK, NT>(dinv, i);
        [[maybe_unused]] Pack<T, PK> wv;
#pragma unroll
        for (int e = 0; e < PK; ++e) wv.v[e] = szero<T>();
        int c = k;
        for (; c + 2 <= s; c += 2) {                                // four basis loads in flight
            const auto g0 = ldp<T, PK, NT>(Gb + (int64_t)c * vs, i), g1 = ldp<T, PK, NT>(Gb + (int64_t)(c + 1) * vs, i);
            [[maybe_unused]] Pack<T, PK> u0, u1;
            if constexpr (MODE != 2) { u0 = ldp<T, PK, NT>(Ub + (int64_t)c * vs, i); u1 = ldp<T, PK, NT>(Ub + (int64_t)(c + 1) * vs, i); }
            const T c0 = cf[c], c1 = cf[c + 1], n0 = sneg(c0), n1 = sneg(c1);
#pragma unroll
            for (int e = 0; e < PK; ++e) {
                vv.v[e] = sadd(sadd(vv.v[e], smul(g0.v[e], n0)), smul(g1.v[e], n1));                 // axpy(-c_i, g_i, v), i ascending
                if constexpr (MODE != 2) wv.v[e] = sadd(sadd(wv.v[e], smul(u0.v[e], c0)), smul(u1.v[e], c1));   // axpy(c_i, u_i, w)
            }
        }
        for (; c < s; ++c) {
            const auto g0 = ldp<T, PK, NT>(Gb + (int64_t)c * vs, i);
            [[maybe_unused]] Pack<T, PK> u0;
            if constexpr (MODE != 2) u0 = ldp<T, PK, NT>(Ub + (int64_t)c * vs, i);
            const T c0 = cf[c], n0 = sneg(c0);
#pragma unroll
            for (int e = 0; e < PK; ++e) {
                vv.v[e] = sadd(vv.v[e], smul(g0.v[e], n0));
                if constexpr (MODE != 2) wv.v[e] = sadd(wv.v[e], smul(u0.v[e], c0));
            }
        }
        if constexpr (MODE != 2) {
#pragma unroll
            for (int e = 0; e < PK; ++e) {
                T vh = vv.v[e];
                if constexpr (MODE == 1) vh = smulv(vh, dv.v[e]);
                vv.v[e] = sadd(smul(vh, om), wv.v[e]);                                               // u_k = vh*omega + w
            }
        }
        stp<T, PK, NT>(out, i, vv);
    }
    __device__ __forceinline__ void epilogue() const {}
};

// ---- IdrsA2 (an applied preconditioner): u_k = vh*omega + sum_{i >= k} u_i c_i, c and omega as IdrsA of this step left them
template <class T>
struct IdrsA2 {
    const IdrsState<T> *S; int s, k; const T *vh; T *Ub; int64_t vs;
    const T *cf; T om;
    __device__ __forceinline__ bool prologue() {
        __shared__ T scT[IDRS_MAXS];
        const int skip = S->hd.skip;
        if ((int)threadIdx.x < IDRS_MAXS) scT[threadIdx.x] = from_dbl<T>(S->c[threadIdx.x]);
        om = from_dbl<T>(S->omega);
        __syncthreads();
        cf = scT;
        return skip == 0;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        auto hv = ldp<T, PK, NT>(vh, i);
        Pack<T, PK> wv;
#pragma unroll
        for (int e = 0; e < PK; ++e) wv.v[e] = szero<T>();
        int c = k;
        for (; c + 4 <= s; c += 4) {                                // four basis loads in flight
            Pack<T, PK> uu[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) uu[q] = ldp<T, PK, NT>(Ub + (int64_t)(c + q) * vs, i);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const T cc = cf[c + q];
#pragma unroll
                for (int e = 0; e < PK; ++e) wv.v[e] = sadd(wv.v[e], smul(uu[q].v[e], cc));
            }
        }
        for (; c < s; ++c) {
            const auto uu = ldp<T, PK, NT>(Ub + (int64_t)c * vs, i);
            const T cc = cf[c];
#pragma unroll
            for (int e = 0; e < PK; ++e) wv.v[e] = sadd(wv.v[e], smul(uu.v[e], cc));
        }
#pragma unroll
        for (int e = 0; e < PK; ++e) hv.v[e] = sadd(smul(hv.v[e], om), wv.v[e]);
        stp<T, PK, NT>(Ub + (int64_t)k * vs, i, hv);
    }
    __device__ __forceinline__ void epilogue() const {}
};

// ---- IdrsB: step k's second half.  q from GmDots' partials (s sums of PQ), alpha, M's column k, beta, F[k + 1]; one pass.
template <class T>
struct IdrsB {
    IdrsState<T> *S; const Dbl<T> *partQ; int64_t qstride; int PQ; int s, k; long long it;
    T *Gb; T *Ub; int64_t vs; T *r; T *x; double *partN;
    const T *cf; T be, nbe; double accN;
    __device__ __forceinline__ bool prologue() {
        using D = Dbl<T>;
        __shared__ D qsum[IDRS_MAXS];
        __shared__ D sM[IDRS_MAXS * IDRS_MAXS], sf[IDRS_MAXS], sa[IDRS_MAXS], smk[IDRS_MAXS], sfn[IDRS_MAXS], sbeta;
        __shared__ T snaT[IDRS_MAXS];
        __shared__ int s_ok;
        __shared__ int s_status;                                    // one read a workgroup: every wavefront takes the same way
        IdrsHead<T> &H = S->hd;
        const int tid = threadIdx.x;
        if (tid == 0) s_status = H.status;                          // requested together with the partials
        if (tid < IDRS_MAXS * IDRS_MAXS && (tid & (IDRS_MAXS - 1)) < k) sM[tid] = (&S->M[0][0])[tid];   // the columns < k
        if (tid < IDRS_MAXS) sf[tid] = S->F[k][tid];
        reduce_coefs(partQ, qstride, PQ, s, qsum);
        if (s_status != ST_RUNNING) return false;
        if (tid == 0) {
            for (int i = 0; i < k; ++i) {                           // M[:k,:k] alpha = q[:k], forward
                D t = qsum[i];
                for (int j = 0; j < i; ++j) t = ssub(t, smul(sM[i * IDRS_MAXS + j], sa[j]));
                sa[i] = sdiv(t, sM[i * IDRS_MAXS + i]);
                snaT[i] = sneg(from_dbl<T>(sa[i]));
            }
            for (int i = k; i < s; ++i) {                           // M[k:,k] = q[k:] - M[k:,:k] alpha
                D m = qsum[i];
                for (int j = 0; j < k; ++j) m = ssub(m, smul(sM[i * IDRS_MAXS + j], sa[j]));
                smk[i] = m;
            }
            const D mkk = smk[k];
            const bool ok = dbl_finite(mkk) && !dbl_is_zero(mkk);
            s_ok = ok ? 1 : 0;
            if (ok) {
                const D beta = sdiv(sf[k], mkk);
                sbeta = beta;
                for (int i = k + 1; i < s; ++i) sfn[i] = ssub(sf[i], smul(beta, smk[i]));
            }
        }
        __syncthreads();
        if (s_ok == 0) {
            if (first_thread()) { H.its = it + 1; H.skip = 1; H.status = ST_BREAKDOWN; }
            return false;
        }
        const D beta = sbeta;
        if (blockIdx.x == 0) {
            if (tid >= k && tid < s) S->M[tid][k] = smk[tid];
            if (tid > k && tid < s) S->F[k + 1][tid] = sfn[tid];
            if (tid == 0) {
                const cplx b2 = cplx{sre(beta), sim(beta)}, m2 = cplx{sre(smk[k]), sim(smk[k])};
                H.its = it + 1; H.kind = k;
                H.tr[0] = b2.re; H.tr[1] = b2.im; H.tr[2] = m2.re; H.tr[3] = m2.im;
            }
        }
        cf = snaT; be = from_dbl<T>(beta); nbe = sneg(be); accN = 0.0;
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto gv = ldp<T, PK, NT>(Gb + (int64_t)k * vs, i); auto uv = ldp<T, PK, NT>(Ub + (int64_t)k * vs, i);
        auto rv = ldp<T, PK, NT>(r, i); auto xv = ldp<T, PK, NT>(x, i);
        int c = 0;
        for (; c + 2 <= k; c += 2) {                                // four basis loads in flight
            const auto g0 = ldp<T, PK, NT>(Gb + (int64_t)c * vs, i), g1 = ldp<T, PK, NT>(Gb + (int64_t)(c + 1) * vs, i);
            const auto u0 = ldp<T, PK, NT>(Ub + (int64_t)c * vs, i), u1 = ldp<T, PK, NT>(Ub + (int64_t)(c + 1) * vs, i);
            const T n0 = cf[c], n1 = cf[c + 1];
#pragma unroll
            for (int e = 0; e < PK; ++e) {
                gv.v[e] = sadd(sadd(gv.v[e], smul(g0.v[e], n0)), smul(g1.v[e], n1));                 // axpy(-alpha_i, g_i, g_k), i ascending
                uv.v[e] = sadd(sadd(uv.v[e], smul(u0.v[e], n0)), smul(u1.v[e], n1));                 // axpy(-alpha_i, u_i, u_k)
            }
        }
        for (; c < k; ++c) {
            const auto g0 = ldp<T, PK, NT>(Gb + (int64_t)c * vs, i); const auto u0 = ldp<T, PK, NT>(Ub + (int64_t)c * vs, i);
            const T n0 = cf[c];
#pragma unroll
            for (int e = 0; e < PK; ++e) {
                gv.v[e] = sadd(gv.v[e], smul(g0.v[e], n0));
                uv.v[e] = sadd(uv.v[e], smul(u0.v[e], n0));
            }
        }
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            const T rr = sadd(rv.v[e], smul(gv.v[e], nbe));                                          // axpy(-beta, g_k, r)
            rv.v[e] = rr;
            xv.v[e] = sadd(xv.v[e], smul(uv.v[e], be));                                              // axpy(beta, u_k, x)
            accN = accN + dbl_sq(rr);
        }
        stp<T, PK, NT>(Gb + (int64_t)k * vs, i, gv);
        stp<T, PK, NT>(Ub + (int64_t)k * vs, i, uv);
        stp<T, PK, NT>(r, i, rv);
        stp<T, PK, NT>(x, i, xv);
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ double smD[NWAVE];
        const double sN = block_sum(accN, smD);
        if (threadIdx.x == 0) partN[blockIdx.x] = sN;
    }
};

// ---- IdrsDots: partials, in the type of the small quantities, of conj(v_b).w for b < nb <= B: one pass over w and the nb vectors
// at V + b * vstride (GmDots' shape; its accumulators are of type T)
template <class T, int B>
struct IdrsDots {
    const IdrsHead<T> *S; const T *V; int64_t vstride; int nb; const T *w; Dbl<T> *part; int64_t pstride;
    Dbl<T> acc[B];
    __device__ __forceinline__ bool prologue() {
        if (S->skip != 0) return false;
#pragma unroll
        for (int b = 0; b < B; ++b) acc[b] = szero<Dbl<T>>();
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        const auto wv = ldp<T, PK, NT>(w, i);
        Pack<T, PK> vv[B];
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (b < nb) vv[b] = ldp<T, PK, NT>(V + (int64_t)b * vstride, i);
#pragma unroll
        for (int b = 0; b < B; ++b)
            if (b < nb) {
#pragma unroll
                for (int e = 0; e < PK; ++e) acc[b] = sadd(acc[b], dbl_cmul(vv[b].v[e], wv.v[e]));
            }
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ Dbl<T> smT[NWAVE];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            if (b < nb) {                                            // (nb is uniform: every thread meets the same barriers)
                const Dbl<T> sum = block_sum(acc[b], smT);
                if (threadIdx.x == 0) part[(int64_t)b * pstride + blockIdx.x] = sum;
            }
        }
    }
};

// ---- IdrsPrec: vh = P r for a diagonal P, the omega step's SpMV input
template <class T, class V>
struct IdrsPrec {
    const IdrsHead<T> *S; const V *dinv; const T *r; T *vh;
    __device__ __forceinline__ bool prologue() const { return S->skip == 0; }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) const {
        auto xv = ldp<T, PK, NT>(r, i); const auto dv = ldp<V, PK, NT>(dinv, i);
#pragma unroll
        for (int e = 0; e < PK; ++e) xv.v[e] = smulv(xv.v[e], dv.v[e]);
        stp<T, PK, NT>(vh, i, xv);
    }
    __device__ __forceinline__ void epilogue() const {}
};

// ---- IdrsW: the omega step.  tt = conj(t).t and tr = conj(t).r from the SpMV's partials (f64 / c64) or from IdrsDots', which holds
// conj(r).t (CONJ_TR) ; omega ; x += vh*omega ; r += t*(-omega) ;
// partials of |r|^2 and (FUSE_F) of f_b = conj(p_b).r on the updated r.  PC: vh is a vector of its own (else it is r).
template <class T, bool PC, bool FUSE_F, bool CONJ_TR>
struct IdrsW {
    IdrsState<T> *S; const Dbl<T> *partTT; const Dbl<T> *partTR; int P; int s; long long it;
    const T *vh; const T *t; const T *Pb; int64_t vs; T *x; T *r; double *partN; Dbl<T> *partF; int64_t fstride;
    T om, nom; double accN; Dbl<T> accF[IDRS_MAXS];
    __device__ __forceinline__ bool prologue() {
        using D = Dbl<T>;
        __shared__ D smT[NWAVE];
        __shared__ D smT2[NWAVE];
        __shared__ int s_status;                                    // one read a workgroup: every wavefront takes the same way
        IdrsHead<T> &H = S->hd;
        if (threadIdx.x == 0) s_status = H.status;                  // requested together with the partials
        const double rn = H.r_norm;
        D tt, tr;
        reduce_partials2(partTT, partTR, P, smT, smT2, tt, tr);
        if (s_status != ST_RUNNING) return false;
        const double ttd = sre(tt);
        const D trd = CONJ_TR ? sconj(tr) : tr;
        const double rho = (double)sabs(trd) / (sqrt(ttd) * rn);
        D omega = smulr(trd, 1.0 / ttd);
        if (rho < IDRS_KAPPA) omega = smulr(omega, IDRS_KAPPA / rho);
        const bool ok = ttd > 0.0 && isfinite(ttd) && dbl_finite(omega) && !dbl_is_zero(omega);
        if (first_thread()) {
            H.its = it + 1;
            if (ok) {
                S->omega = omega; H.kind = s;
                H.tr[0] = sre(omega); H.tr[1] = sim(omega); H.tr[2] = ttd; H.tr[3] = 0.0;
            } else { H.skip = 1; H.status = ST_BREAKDOWN; }
        }
        if (!ok) return false;
        om = from_dbl<T>(omega); nom = sneg(om); accN = 0.0;
#pragma unroll
        for (int b = 0; b < IDRS_MAXS; ++b) accF[b] = szero<D>();
        return true;
    }
    template <int PK, bool NT> __device__ __forceinline__ void run(int64_t i) {
        auto xv = ldp<T, PK, NT>(x, i); auto rv = ldp<T, PK, NT>(r, i); const auto tv = ldp<T, PK, NT>(t, i);
        Pack<T, PK> hv = rv;
        if constexpr (PC) hv = ldp<T, PK, NT>(vh, i);
        [[maybe_unused]] Pack<T, PK> pv[IDRS_MAXS];
        if constexpr (FUSE_F) {
#pragma unroll
            for (int b = 0; b < IDRS_MAXS; ++b)
                if (b < s) pv[b] = ldp<T, PK, NT>(Pb + (int64_t)b * vs, i);
        }
#pragma unroll
        for (int e = 0; e < PK; ++e) {
            xv.v[e] = sadd(xv.v[e], smul(hv.v[e], om));                                              // axpy(omega, vh, x)
            const T rr = sadd(rv.v[e], smul(tv.v[e], nom));                                          // axpy(-omega, t, r)
            rv.v[e] = rr;
            accN = accN + dbl_sq(rr);
        }
        stp<T, PK, NT>(x, i, xv);
        stp<T, PK, NT>(r, i, rv);
        if constexpr (FUSE_F) {
#pragma unroll
            for (int b = 0; b < IDRS_MAXS; ++b)
                if (b < s) {
#pragma unroll
                    for (int e = 0; e < PK; ++e) accF[b] = sadd(accF[b], dbl_cmul(pv[b].v[e], rv.v[e]));
                }
        }
    }
    __device__ __forceinline__ void epilogue() {
        __shared__ double smD[NWAVE];
        __shared__ Dbl<T> smF[NWAVE];
        const double sN = block_sum(accN, smD);
        if (threadIdx.x == 0) partN[blockIdx.x] = sN;
        if constexpr (FUSE_F) {
#pragma unroll
            for (int b = 0; b < IDRS_MAXS; ++b) {
                if (b < s) {                                         // (s is uniform: every thread meets the same barriers)
                    const Dbl<T> sF = block_sum(accF[b], smF);
                    if (threadIdx.x == 0) partF[(int64_t)b * fstride + blockIdx.x] = sF;
                }
            }
        }
    }
};

// idrs_check (one workgroup): the events of the step whose IdrsB left partN — before the omega step, and behind the last
// product a solve enqueues.  PN == 0: no step ran yet, |r|^2 is the host's r0sq.
template <class T>
__global__ __launch_bounds__(BLOCK) void idrs_check_kernel(IdrsState<T> *S, const double *partN, int PN, long long it) {
    __shared__ double smD[NWAVE];
    IdrsHead<T> &H = S->hd;
    const int status = H.status;
    const double tol2 = H.tol2, r0sq = H.r0sq;
    const long long max_iter = H.max_iter;
    const double sN = PN > 0 ? reduce_partials(partN, PN, smD) : r0sq;
    if (status != ST_RUNNING) return;
    (void)idrs_decide<T>(&H, sN, tol2, max_iter, it);
}

}  // namespace sprs
